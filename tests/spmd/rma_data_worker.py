"""SPMD worker: the RMA data paths at the counts, chunk seams and alignments
of tests/spmd/rma_data_cases.py (the plan and the model), on device windows.

Rank r targets (r + 1) % n.  One window per element type is created once and
refilled before every epoch; every target range has sentinel guards on both
sides, every origin and result buffer is a view inside a larger allocation
with guards.  After each epoch the ENTIRE window (as target) and the entire
result allocation (as origin) are compared with the model, bit for bit
(golden_io.same_bits' any-NaN rule for bf16 only).  RMA_DATA_SECTIONS names
the plan's sections.  Prints one JSON line {"rank", "ran", "nfail",
"first_failures", ...}.  Launched by tests/test_rma_data_gpu.py.

Reference calls: src/onesided.jl:150-219 (Get, Put, Fetch_and_op, Accumulate,
Get_accumulate), :124-148 (fence, lock, unlock)."""
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
import torch  # noqa: E402

import mpigx as MPI  # noqa: E402
import rma_data_cases as C  # noqa: E402
from golden_io import same_bits  # noqa: E402

T0 = time.time()
comm = MPI.Init()
rank, n = MPI.Comm_rank(comm), MPI.Comm_size(comm)
tgt, src = (rank + 1) % n, (rank - 1) % n
DEV = f"cuda:{comm.device}"
SCRATCH = int(os.environ.get("MPIGX_RMA_SCRATCH", C.DEFAULT_SCRATCH))
EPOCHS = C.plan(n, os.environ["RMA_DATA_SECTIONS"].split(","), SCRATCH)
G = C.GUARD
MPI_ERR_OP = 9

FAILS = []   # {"case", "part", "index", "got", "want"}
BAD = set()  # ids of cases with a failing part
RAN = 0


def seed_of(c, origin):
    return c["seed"] * 64 + origin


def tdt(tname):
    return getattr(torch, tname)


def first_diff(got, exp, bf16):
    """None when equal, else (element index, got bits, wanted bits)."""
    if got.shape == exp.shape and (same_bits(got, exp, bf16=True) if bf16 else
                                   np.array_equal(got.view(np.uint8), exp.view(np.uint8))):
        return None
    if got.shape != exp.shape:
        return (-1, f"shape {got.shape}", f"shape {exp.shape}")
    w = min(got.dtype.itemsize, 8)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w]
    a, b = got.view(u), exp.view(u)
    ne = a != b
    if bf16:
        ne &= ~(((a & 0x7FFF) > 0x7F80) & ((b & 0x7FFF) > 0x7F80))
    i = int(np.flatnonzero(ne)[0])
    return (i * w // got.dtype.itemsize, format(int(a[i]), "x"), format(int(b[i]), "x"))


def fail(c, part, d):
    BAD.add(c["id"])
    FAILS.append({"case": c["id"], "part": part, "index": d[0], "got": d[1], "want": d[2]})


def err_class(fn):
    try:
        fn()
    except MPI.MPIError as e:
        return MPI.Error_class(e.code)
    return 0


class Guarded:
    """`payload` (typed numpy) on the device at `off` bytes past a RES_GUARD
    inside a sentinel-filled allocation; `.view` is the typed device view."""

    def __init__(self, payload, tname, off=0):
        raw = payload.view(np.uint8).reshape(-1)
        self.lo = C.RES_GUARD + off
        self.host = np.full(self.lo + raw.size + C.RES_GUARD, C.SENTINEL, np.uint8)
        self.host[self.lo:self.lo + raw.size] = raw
        self.alloc = torch.from_numpy(self.host.copy()).to(DEV)
        assert self.alloc.data_ptr() % 16 == 0
        self.nb, self.tname = raw.size, tname
        self.view = self.alloc[self.lo:self.lo + raw.size].view(tdt(tname))

    def check(self, c, part, payload):
        """The whole allocation: guards untouched, payload as modelled."""
        got = self.alloc.cpu().numpy()
        want = self.host.copy()
        want[self.lo:self.lo + self.nb] = payload.view(np.uint8).reshape(-1)
        dt = C.npdt(self.tname)
        d = first_diff(got[self.lo:self.lo + self.nb].view(dt), want[self.lo:self.lo + self.nb].view(dt),
                       self.tname == "bfloat16")
        if d:
            fail(c, part, d)
        got[self.lo:self.lo + self.nb] = want[self.lo:self.lo + self.nb]
        d = first_diff(got, want, False)
        if d:
            fail(c, part + " guard", d)


class Window:
    def __init__(self, tname, length):
        self.tname, self.length = tname, length
        self.raw = torch.empty(length * C.esize(tname), dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.win = MPI.Win_create(self.raw.view(tdt(tname)), comm)
        self.exp = C.sentinel(tname, length)
        self.dirty = length  # elements from the start that may not hold the sentinel on the device

    def fill(self, init):
        """Refill: `init`, then sentinels to the end.  Past the previous
        epoch's extent the device already holds the sentinel (its whole-window
        comparison passed), so only the prefix is rebuilt and uploaded.
        Returns the host model of the whole window."""
        hi = max(self.dirty, init.size)
        self.exp.view(np.uint8)[:hi * C.esize(self.tname)] = C.SENTINEL
        self.exp[:init.size] = init
        nb = hi * C.esize(self.tname)
        self.raw[:nb].copy_(torch.from_numpy(self.exp.view(np.uint8)[:nb]))
        self.dirty = init.size
        return self.exp

    def read(self):
        return self.raw.cpu().numpy().view(C.npdt(self.tname))

    def free(self):
        MPI.free(self.win)


def begin(sync, win, lock=None):
    torch.cuda.synchronize()
    if sync == "fence":
        MPI.Win_fence(0, win)
    else:
        MPI.Barrier(comm)
        MPI.Win_lock(lock or MPI.LOCK_EXCLUSIVE, tgt, 0, win)


def end(sync, win):
    if sync == "fence":
        MPI.Win_fence(0, win)
    else:
        MPI.Win_unlock(tgt, win)
        MPI.Barrier(comm)
    torch.cuda.synchronize()


def check_window(ep, W, exp):
    """Entire window against the model; a difference is charged to the case
    whose range or guards hold it."""
    got = W.read()
    bf = W.tname == "bfloat16"
    if first_diff(got, exp, bf) is None:
        return
    W.dirty = W.length  # the device's content is unknown: the next refill uploads everything
    found = False
    bounds = [c.get("at", G) - G for c in ep["cases"]][1:] + [W.length]
    for c, hi in zip(ep["cases"], bounds):
        lo = c.get("at", G) - G
        d = first_diff(got[lo:hi], exp[lo:hi], bf)
        if d:
            found = True
            fail(c, "window", (d[0] - G, d[1], d[2]))  # index relative to the case's range
    if not found:
        fail(ep["cases"][0], "window outside every range", first_diff(got, exp, bf))


def run_disjoint(ep, W):
    tn, win = ep["type"], W.win
    init = C.sentinel(tn, ep["length"])
    as_target = []
    for c in ep["cases"]:
        at = c["at"]
        if c["kind"] in ("put", "get"):
            pay = C.byte_payload(c["nbytes"], seed_of(c, src))
            if c["kind"] == "get":
                init[at + c["src_mod"]:at + c["src_mod"] + c["nbytes"]] = pay
            as_target.append(pay)
        else:
            w, o = C.operand_pair(tn, c["op"], c["count"], seed_of(c, src))
            init[at:at + c["count"]] = w
            as_target.append((w, o[:c["count"]]))
    exp = W.fill(init)
    issued = []
    for c in ep["cases"]:
        if c["kind"] == "put":
            issued.append((Guarded(C.byte_payload(c["nbytes"], seed_of(c, rank)), tn, c["src_mod"]), None, None))
        elif c["kind"] == "get":
            issued.append((None, Guarded(C.sentinel(tn, c["nbytes"]), tn, c["dst_mod"]),
                           C.byte_payload(c["nbytes"], seed_of(c, rank))))
        else:
            w, o = C.operand_pair(tn, c["op"], c["count"], seed_of(c, rank))
            res = Guarded(C.sentinel(tn, c["count"]), tn) if c["kind"] != "acc" else None
            issued.append((Guarded(o[:c["count"]], tn, c["ooff"]), res, w))
    begin(ep["sync"], win)
    rcs = []
    for c, (ob, rb, _) in zip(ep["cases"], issued):
        k, at = c["kind"], c["at"]
        if k == "put":
            rcs.append(err_class(lambda: MPI.Put(ob.view, c["nbytes"], tgt, at + c["dst_mod"], win)))
        elif k == "get":
            rcs.append(err_class(lambda: MPI.Get(rb.view, c["nbytes"], tgt, at + c["src_mod"], win)))
        elif k == "acc":
            rcs.append(err_class(lambda: MPI.Accumulate(ob.view, c["count"], tgt, at, getattr(MPI, c["op"]), win)))
        elif k == "gacc":
            rcs.append(err_class(lambda: MPI.Get_accumulate(ob.view, rb.view, c["count"], tgt, at,
                                                            getattr(MPI, c["op"]), win)))
        else:
            rcs.append(err_class(lambda: MPI.Fetch_and_op(ob.view, rb.view, tgt, at, getattr(MPI, c["op"]), win)))
    end(ep["sync"], win)
    # as target: the whole window
    for c, val in zip(ep["cases"], as_target):
        at = c["at"]
        if c["kind"] == "put":
            exp[at + c["dst_mod"]:at + c["dst_mod"] + c["nbytes"]] = val
        elif c["kind"] != "get" and not (c["kind"] == "acc" and c["op"] == "NO_OP"):
            exp[at:at + c["count"]] = C.model(tn, val[0], val[1], c["op"])[0]
    check_window(ep, W, exp)
    # as origin: return codes, whole result allocations, origin allocations unchanged
    for c, rc, (ob, rb, old) in zip(ep["cases"], rcs, issued):
        want_rc = MPI_ERR_OP if (c["kind"] == "acc" and c["op"] == "NO_OP") else 0  # MPI_NO_OP only fetches
        if rc != want_rc:
            fail(c, "rc", (0, str(rc), str(want_rc)))
        if rb is not None:
            rb.check(c, "result", old)
        if ob is not None:
            ob.check(c, "origin", ob.host[ob.lo:ob.lo + ob.nb].copy())


def run_order(ep, W):
    tn, win, c = ep["type"], W.win, ep["cases"][0]
    dt, span = C.npdt(tn), ep["length"] - 2 * G

    def base(who):
        rng = np.random.default_rng([c["seed"], who, 79])
        return (rng.integers(-4, 5, span) * 0.5).astype(dt) if dt.kind == "f" else rng.integers(-9, 10, span).astype(dt)

    init = C.sentinel(tn, ep["length"])
    init[G:G + span] = base(src)
    exp = W.fill(init)
    ops = [C.order_operand(tn, j, seed_of(c, rank)) for j in range(C.ORDER_POSTS)]
    ob = Guarded(np.concatenate([o for _, o in ops]), tn, C.origin_off(tn, 1))
    begin(ep["sync"], win)
    for j, ((op, _), s) in enumerate(zip(ops, C.order_starts())):
        MPI.Accumulate(ob.view[j * C.ORDER_COUNT:(j + 1) * C.ORDER_COUNT], C.ORDER_COUNT, tgt, G + s,
                       getattr(MPI, op), win)
    end(ep["sync"], win)
    for j, s in enumerate(C.order_starts()):  # program order of my origin
        op, o = C.order_operand(tn, j, seed_of(c, src))
        exp[G + s:G + s + C.ORDER_COUNT] = C.model(tn, exp[G + s:G + s + C.ORDER_COUNT].copy(), o, op)[0]
    check_window(ep, W, exp)


def run_multi(ep, W):
    tn, win, c = ep["type"], W.win, ep["cases"][0]
    init = C.sentinel(tn, ep["length"])
    at = [G + k * (C.ORDER_COUNT + G) for k in range(len(C.MULTI_OPS))]
    rng = np.random.default_rng([c["seed"], 80])
    for a in at:
        init[a:a + C.ORDER_COUNT] = rng.integers(-5, 6, C.ORDER_COUNT)
    exp = W.fill(init)
    ops = [C.multi_operand(j, rank) for j in range(C.MULTI_POSTS)]
    ob = Guarded(np.concatenate([o for _, o in ops]), tn)
    begin("fence", win)
    for j, (op, _) in enumerate(ops):
        MPI.Accumulate(ob.view[j * C.ORDER_COUNT:(j + 1) * C.ORDER_COUNT], C.ORDER_COUNT, 0,
                       at[j % len(at)], getattr(MPI, op), win)
    end("fence", win)
    if rank == 0:  # any arrival order gives the same window
        for who in range(n):
            for j in range(C.MULTI_POSTS):
                op, o = C.multi_operand(j, who)
                a = at[j % len(at)]
                exp[a:a + C.ORDER_COUNT] = C.model(tn, exp[a:a + C.ORDER_COUNT].copy(), o, op)[0]
    check_window(ep, W, exp)


def main():
    global RAN
    per = {}
    for tn in dict.fromkeys(ep["type"] for ep in EPOCHS):
        W = Window(tn, C.window_elems(EPOCHS, tn))
        for ep in EPOCHS:
            if ep["type"] != tn:
                continue
            for c in ep["cases"]:
                if "per" in c:  # the seams this plan assumes are the engine's
                    assert c["per"] == C.seam_per(SCRATCH, n, C.esize(tn)), (c["per"], SCRATCH, n)
                    per[tn] = c["per"]
            {"disjoint": run_disjoint, "order": run_order, "multi": run_multi}[ep["shape"]](ep, W)
            RAN += len(ep["cases"])
        MPI.Barrier(comm)
        W.free()
    return per


failed, per = None, {}
try:
    per = main()
except Exception:  # noqa: BLE001
    failed = traceback.format_exc()
print(json.dumps({"rank": rank, "n": n, "ran": RAN, "planned": C.ncases(EPOCHS), "nfail": len(BAD) + (failed is not None),
                  "first_failures": FAILS[:8], "failed": failed, "per": per, "scratch": SCRATCH,
                  "seconds": round(time.time() - T0, 2)}), flush=True)
if failed is None:
    MPI.Finalize()
sys.exit(1 if failed else 0)
