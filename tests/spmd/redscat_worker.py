"""SPMD worker of tests/test_redscat_gpu.py (one process per rank): Reduce_scatter_block
and Reduce_scatter on device buffers, every check bit-exact.  RS_PHASE picks
the cases:
  golden  every fixture case recorded from MPICH at this world size
          (tests/golden/redscat_golden*.npz), on the staged path and, with
          RS_ZC=1, again through the zero-copy kernel (ZC_MIN=1, ZC_REQUIRE=1)
  big     1 Mi + 3 elements per block, FLOAT SUM and INT64_T BAND, block and v
          forms, in place and out of place, against the model; staged (the
          launcher passes a small MPIGX_STAGING_BYTES: several rounds), then
          zero-copy
  misc    LINEAR order, bf16, a contiguous derived type, a non-commutative
          user op through both registration calls, the error classes
  xdev    3 and 16384 per block FLOAT SUM on both paths (the launcher sets
          MPIGX_PEER_MEM=xdev)
  stream  stream-ordered mode: two back-to-back calls on a side stream behind
          a producer kernel, then mpigx_comm_synchronize
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

import mpigx as MPI  # noqa: E402
import redscat_model as R  # noqa: E402
from oracle import mpich_model as M  # noqa: E402

IN_PLACE = ctypes.c_void_p(-1 & ((1 << 64) - 1))
PHASE = os.environ.get("RS_PHASE", "golden")

comm = MPI.Init()
L = MPI.lib()
r, n, cv = MPI.Comm_rank(comm), MPI.Comm_size(comm), comm.val
FAIL, RAN = [], [0]
_KEEP = []


def check(ok, what):
    RAN[0] += 1
    if not ok:
        FAIL.append(what)


def dev(a):
    """`a`'s bytes in a device allocation of its own (+64 B so that an empty
    array still has an address), kept alive until the next call."""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    t = torch.empty(raw.size + 64, dtype=torch.uint8, device="cuda")[: raw.size]
    t.copy_(torch.from_numpy(raw.copy()))
    _KEEP.append(t)
    return t


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def same(a, b):
    """Bitwise; any NaN matches any NaN (tests/golden_io.py same_bits)."""
    if a.shape != b.shape:
        return False
    if a.dtype.kind in "fc":
        fa, fb = a.view(a.real.dtype), b.view(b.real.dtype)
        na, nb = np.isnan(fa), np.isnan(fb)
        return np.array_equal(na, nb) and fa[~na].tobytes() == fb[~nb].tobytes()
    return a.tobytes() == b.tobytes()


def run(x, counts, dtname, opname, v, inplace, npdt=None, handle=None, op=None):
    """One call on my sendbuf x; returns my block (numpy)."""
    _KEEP.clear()
    npdt = npdt or M.DTYPES[dtname][1]
    h = handle if handle is not None else M.DTYPES[dtname][0]
    o = op if op is not None else M.OPS[opname]
    mine = counts[r]
    es = np.dtype(npdt).itemsize
    if inplace:
        recv, send = dev(x), IN_PLACE
    else:
        recv, send = dev(np.full(mine * es, 0xCD, np.uint8)), P(dev(x))
    if v:
        rc = L.mpigx_reduce_scatter(send, P(recv), (ctypes.c_int * n)(*counts), h, o, cv)
    else:
        rc = L.mpigx_reduce_scatter_block(send, P(recv), counts[0], h, o, cv)
    assert rc == 0, (rc, dtname, opname, counts, v, inplace)
    return recv.cpu().numpy()[: mine * es].view(npdt)


def zero_copy(on):
    MPI.set_knob(comm, "ZC_MIN", 1 if on else ZC_MIN0)
    MPI.set_knob(comm, "ZC_REQUIRE", 1 if on else 0)


ZC_MIN0 = MPI.get_knob(comm, "ZC_MIN")


def golden(tag):
    cases, arrays = R.load_golden()
    cases = [c for c in cases if c["n"] == n]
    assert len(cases) > 90
    for c in cases:
        counts = R.counts_of(c, n)
        x = R.gen_input(c["dtype"], sum(counts), r, n, c["seed"], c["mode"])
        got = run(x, counts, c["dtype"], c["op"], c["v"], c["inplace"])
        want = R.split_outputs(c, arrays[c["id"]])[r]
        check(same(R.sample(got, c), want), (tag, c["id"]))


def big(tag):
    base = (1 << 20) + 3
    rng = np.random.default_rng(11)  # the same stream on every rank: everyone holds all inputs
    for dtname, opname in (("FLOAT", "SUM"), ("INT64_T", "BAND")):
        for v in (0, 1):
            counts = [base + (q % 3) - 1 for q in range(n)] if v else [base] * n
            tot = sum(counts)
            if dtname == "FLOAT":
                ins = [np.ldexp(rng.uniform(-1, 1, tot), rng.integers(-8, 8, tot)).astype(np.float32) for _ in range(n)]
            else:
                ins = [rng.integers(-(1 << 62), 1 << 62, tot, dtype=np.int64) | rng.integers(0, 1 << 62, tot, dtype=np.int64)
                       for _ in range(n)]
            want = R.reduce_scatter(ins, counts, dtname, opname)[r]
            for inplace in (0, 1):
                got = run(ins[r], counts, dtname, opname, v, inplace)
                check(same(got, want), (tag, dtname, opname, "v" if v else "block", "ip" if inplace else "oop"))
    # In place with strongly unequal counts on a grid of many blocks: what block b of a rank stores
    # into the start of its buffer is input that OTHER blocks still read (block b - 1 of the same
    # rank for counts [1, M, ...]; block 0 of the next owner), ordered only by a whole-launch barrier.
    for counts in ([1] + [base + q for q in range(1, n)], [base + q for q in range(1, n)] + [1]):
        tot = sum(counts)
        ins = [np.ldexp(rng.uniform(-1, 1, tot), rng.integers(-8, 8, tot)).astype(np.float32) for _ in range(n)]
        want = R.reduce_scatter(ins, counts, "FLOAT", "SUM")[r]
        for rep in range(3):
            check(same(run(ins[r], counts, "FLOAT", "SUM", 1, 1), want), (tag, "unequal-ip", counts[0], rep))


def misc():
    rng = np.random.default_rng(23)
    counts = [5, 0, 9]
    tot = sum(counts)
    ins = [np.ldexp(rng.uniform(-1, 1, tot), rng.integers(-8, 8, tot)).astype(np.float32) for _ in range(n)]
    bl = [np.ldexp(rng.uniform(-1, 1, 7 * n), rng.integers(-8, 8, 7 * n)).astype(np.float32) for _ in range(n)]
    # MPIGX_ORDER_LINEAR = the LINEAR Allreduce, sliced
    MPI.set_reduce_order(comm, 1)
    full = M.fold_linear(ins, "FLOAT", "SUM")
    at = sum(counts[:r])
    for zc in (0, 1):
        zero_copy(zc)
        check(same(run(ins[r], counts, "FLOAT", "SUM", 1, 0), full[at:at + counts[r]]), ("linear-v", zc))
        check(same(run(bl[r], [7] * n, "FLOAT", "SUM", 0, 1), M.fold_linear(bl, "FLOAT", "SUM")[7 * r:7 * r + 7]),
              ("linear-block-ip", zc))
    MPI.set_reduce_order(comm, 0)
    # bf16 against the model (MPICH has no bf16: parity unpinned)
    bcounts = [33, 8, 17]
    bins = [M.f32_to_bf16(rng.uniform(-4, 4, sum(bcounts)).astype(np.float32)) for _ in range(n)]
    bins[1][::5] = M.f32_to_bf16(np.array([np.nan], np.float32))[0]
    for zc in (0, 1):
        zero_copy(zc)
        for opname in ("SUM", "MAX"):
            want = R.reduce_scatter(bins, bcounts, "BFLOAT16", opname)[r]
            got = run(bins[r], bcounts, "BFLOAT16", opname, 1, 0)
            f = lambda u: (u.astype(np.uint32) << 16).view(np.float32)  # noqa: E731
            check(same(f(got), f(want)), ("bf16", opname, zc))
    # a contiguous derived type of 4 FLOATs: counts are in instances
    quad = MPI.Types.commit_(MPI.Types.create_contiguous(4, MPI.Datatype(np.float32)))
    qc = [2, 1, 3]
    qins = [np.ldexp(rng.uniform(-1, 1, 4 * sum(qc)), rng.integers(-8, 8, 4 * sum(qc))).astype(np.float32) for _ in range(n)]
    for zc in (0, 1):
        zero_copy(zc)
        want = R.reduce_scatter(qins, [4 * c for c in qc], "FLOAT", "SUM")[r]
        x = torch.from_numpy(qins[r]).cuda()
        y = torch.zeros(4 * qc[r], dtype=torch.float32, device="cuda")
        MPI.Reduce_scatter_(MPI.Buffer(x, sum(qc), quad), MPI.Buffer(y, qc[r], quad), qc, MPI.SUM, comm)
        check(same(y.cpu().numpy(), want), ("derived-v", zc))
        want = R.reduce_scatter([q[:24] for q in qins], [8] * n, "FLOAT", "SUM")[r]
        y = torch.zeros(8, dtype=torch.float32, device="cuda")
        MPI.Reduce_scatter_block_(MPI.Buffer(x, 6, quad), MPI.Buffer(y, 2, quad), 2, MPI.SUM, comm)
        check(same(y.cpu().numpy(), want), ("derived-block", zc))
    zero_copy(0)
    # the allocating form and an opfunc callable (routed like Allreduce_'s)
    xi = torch.arange(6, dtype=torch.int64, device="cuda") * (r + 1)
    yi = MPI.Reduce_scatter_block(xi, MPI.SUM, comm)
    check(yi.cpu().tolist() == [6 * (2 * r), 6 * (2 * r + 1)], "allocating")
    yi = torch.zeros(2, dtype=torch.int64, device="cuda")
    MPI.Reduce_scatter_block_(xi, yi, lambda a, b: a + b, comm)
    check(yi.cpu().tolist() == [6 * (2 * r), 6 * (2 * r + 1)], "opfunc")
    user_ops(rng)
    errors()


def compose_np(x, y):
    """in o inout for affine maps (a, b) o (c, d) = (a c, a d + b) on wrapping int64 pairs."""
    xv, yv = x.reshape(-1, 2), y.reshape(-1, 2)
    with np.errstate(over="ignore"):
        return np.stack([xv[:, 0] * yv[:, 0], xv[:, 0] * yv[:, 1] + xv[:, 1]], axis=1).reshape(-1)


def compose_t(x, y):
    xv, yv = x.reshape(-1, 2), y.reshape(-1, 2)
    return torch.stack([xv[:, 0] * yv[:, 0], xv[:, 0] * yv[:, 1] + xv[:, 1]], dim=1).reshape(-1)


_cb_keep = []


def host_cb_op(fn):
    from mpigx._lib import USER_FN

    def cb(invec, inoutvec, plen, pdt):
        sz = ctypes.c_longlong(0)
        L.mpigx_type_size_x(pdt[0], ctypes.byref(sz))
        nb = plen[0] * sz.value
        a = np.ctypeslib.as_array((ctypes.c_char * nb).from_address(invec)).view(np.int64)
        b = np.ctypeslib.as_array((ctypes.c_char * nb).from_address(inoutvec)).view(np.int64)
        b[:] = fn(a, b)

    f = USER_FN(cb)
    h = ctypes.c_int(0)
    assert L.mpigx_op_create(f, 0, ctypes.byref(h)) == 0
    _cb_keep.append(f)
    return MPI.Op(None, _val=h.value, _name="hostcb")


def user_ops(rng):
    """Associative, not commutative: every block folded in rank order (x0 o (x1 o x2))."""
    pair = MPI.Types.commit_(MPI.Types.create_contiguous(2, MPI.Datatype(np.int64)))
    counts = [3, 0, 4]  # pairs per block
    tot = sum(counts)
    ins = [rng.integers(-(1 << 40), 1 << 40, 2 * tot, dtype=np.int64) for _ in range(n)]
    acc = ins[n - 1].copy()
    for q in range(n - 2, -1, -1):
        acc = compose_np(ins[q], acc)
    at = 2 * sum(counts[:r])
    want = acc[at:at + 2 * counts[r]]
    bins = [rng.integers(-(1 << 40), 1 << 40, 2 * 3 * n, dtype=np.int64) for _ in range(n)]  # 3 pairs per block
    bacc = bins[n - 1].copy()
    for q in range(n - 2, -1, -1):
        bacc = compose_np(bins[q], bacc)
    for name, op in (("op_create", host_cb_op(compose_np)), ("op_create_device", MPI.Op(compose_t, np.int64))):
        x = torch.from_numpy(ins[r]).cuda()
        y = torch.zeros(2 * counts[r] + 2, dtype=torch.int64, device="cuda")
        MPI.Reduce_scatter_(MPI.Buffer(x, tot, pair), MPI.Buffer(y, counts[r], pair), counts, op, comm)
        check(y.cpu().numpy()[: 2 * counts[r]].tobytes() == want.tobytes(), ("userop-v", name))
        if op.val is not None:  # aliased out-of-place buffers are refused with a user op too
            xa = dev(np.zeros(64, np.int64))
            check(L.mpigx_reduce_scatter_block(P(xa), P(xa), 2, M.DTYPES["INT64_T"][0], op.val, cv)
                  == MPI.consts.MPI_ERR_BUFFER, ("userop-alias", name))
        z = torch.from_numpy(bins[r]).cuda()  # in place
        MPI.Reduce_scatter_block_(MPI.Buffer(z, 3 * n, pair), 3, op, comm)
        check(z.cpu().numpy()[:6].tobytes() == bacc[6 * r:6 * r + 6].tobytes(), ("userop-block-ip", name))


def errors():
    """Every rank passes the same bad arguments: the error class comes back on
    every rank and the communicator still works afterwards."""
    x = dev(np.zeros(64, np.float32))
    y = dev(np.zeros(64, np.float32))
    F, S = M.DTYPES["FLOAT"][0], M.OPS["SUM"]
    check(L.mpigx_reduce_scatter_block(P(x), P(y), -1, F, S, cv) == MPI.consts.MPI_ERR_COUNT, "err-count-block")
    check(L.mpigx_reduce_scatter(P(x), P(y), (ctypes.c_int * n)(1, -2, 1), F, S, cv) == MPI.consts.MPI_ERR_COUNT,
          "err-count-v")
    check(L.mpigx_reduce_scatter_block(P(x), P(y), 2, F, M.OPS["BAND"], cv) == MPI.consts.MPI_ERR_OP, "err-op")
    check(L.mpigx_reduce_scatter_block(P(x), P(y), 2, 1, S, cv) == MPI.consts.MPI_ERR_TYPE, "err-type")
    check(L.mpigx_reduce_scatter_block(P(x), P(x), 2, F, S, cv) == MPI.consts.MPI_ERR_BUFFER, "err-alias")
    check(L.mpigx_reduce_scatter_block(None, P(y), 2, F, S, cv) == MPI.consts.MPI_ERR_BUFFER, "err-null")
    check(L.mpigx_reduce_scatter_block(P(x), P(y), 0, F, S, cv) == 0, "zero-total")
    check(L.mpigx_reduce_scatter(P(x), P(y), (ctypes.c_int * n)(0, 0, 0), F, S, cv) == 0, "zero-total-v")
    # a rank that passes other counts than its peers: every rank gets MPI_ERR_COUNT, nobody launches
    odd = (ctypes.c_int * n)(2, 2, 3 if r == 1 else 2)
    check(L.mpigx_reduce_scatter(P(x), P(y), odd, F, S, cv) == MPI.consts.MPI_ERR_COUNT, "err-count-mismatch")
    ins = [np.full(6, q + 1, np.float32) for q in range(n)]
    check(same(run(ins[r], [2] * n, "FLOAT", "SUM", 0, 0), np.full(2, 6, np.float32)), "after-errors")


def xdev():
    pm = MPI.peer_memory(comm)
    for zc in (0, 1):
        zero_copy(zc)
        for k, count in enumerate((3, 16384)):
            c = {"n": n, "dtype": "FLOAT", "count": count, "v": 0, "seed": 7700 + k, "mode": R.G_WIDE}
            ins = R.case_inputs(c)
            want = R.reduce_scatter(ins, [count] * n, "FLOAT", "SUM")[r]
            check(same(run(ins[r], [count] * n, "FLOAT", "SUM", 0, 0), want), ("xdev", count, zc, str(pm)))


def stream():
    """Stream-ordered: the producer kernel, two calls and nothing else between
    them on a side stream; the second call's input is the first one's output."""
    count = 4096
    c = {"n": n, "dtype": "FLOAT", "count": count, "v": 0, "seed": 7800, "mode": R.G_WIDE}
    ins = R.case_inputs(c)
    first = R.reduce_scatter([2 * x for x in ins], [count] * n, "FLOAT", "SUM")
    half = count // n
    second = R.reduce_scatter(first, [half] * n, "FLOAT", "SUM")[r]
    for zc in (0, 1):
        zero_copy(zc)
        side = torch.cuda.Stream()
        x = torch.from_numpy(ins[r]).cuda()
        y = torch.zeros(count, dtype=torch.float32, device="cuda")
        z = torch.zeros(half, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert L.mpigx_comm_set_blocking(cv, 0) == 0
        with torch.cuda.stream(side):
            x.mul_(2)  # producer
            MPI.Reduce_scatter_block_(x, y, count, MPI.SUM, comm)
            MPI.Reduce_scatter_block_(y, z, half, MPI.SUM, comm)
            assert L.mpigx_comm_synchronize(cv) == 0
        assert L.mpigx_comm_set_blocking(cv, 1) == 0
        check(same(y.cpu().numpy(), first[r]), ("stream-first", zc))
        check(same(z.cpu().numpy(), second), ("stream-second", zc))
    zero_copy(0)


if PHASE == "golden":
    golden("staged")
    if os.environ.get("RS_ZC") == "1":
        zero_copy(1)
        golden("zc")
elif PHASE == "big":
    big("staged")
    zero_copy(1)
    big("zc")
elif PHASE == "misc":
    misc()
elif PHASE == "xdev":
    xdev()
elif PHASE == "stream":
    stream()
else:
    raise SystemExit(f"unknown RS_PHASE {PHASE}")

hits, exch = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
L.mpigx_comm_zc_stats(cv, ctypes.byref(hits), ctypes.byref(exch))
MPI.Finalize()
print(json.dumps({"rank": r, "n": n, "phase": PHASE, "checks": RAN[0], "nfail": len(FAIL),
                  "failures": [str(f) for f in FAIL[:12]], "zc_exchanges": exch.value}), flush=True)
sys.exit(1 if FAIL else 0)
