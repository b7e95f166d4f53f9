"""SPMD parity worker (one process per rank; the reference's test strategy:
test/runtests.jl runs each test_*.jl under `mpiexec -n nprocs`).

Runs every MPICH golden case recorded at this world size through libmpigx's
C ABI on device buffers (both algorithms, in-place forms, both reduce
orders), plus larger seeded cases checked against the oracle, and exits
non-zero on any mismatch.  Launched by tests/test_collectives_gpu.py.

GOLDEN_PASSES lists the passes of one launch: "staged", "zc" (every size
through the zero-copy paths, MPIGX_ZC_MIN=1 MPIGX_ZC_REQUIRE=1) or
"staged,zc".  A pass whose path the launch's environment already selects runs
on COMM_WORLD; the zero-copy pass after a staged one runs on a Comm_dup made
once every rank has put the two settings into its environment (a communicator
reads its path-selecting settings when it is created).  Each pass runs the
phases its own launch would and prints its own summary line.  Without
GOLDEN_PASSES the launch is one pass, "zc" if MPIGX_ZC_MIN is set.
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
from gen_inputs import make  # noqa: E402
from golden_io import load, same_bits, typed  # noqa: E402
from oracle import mpich_model as M  # noqa: E402

IN_PLACE = ctypes.c_void_p(-1 & ((1 << 64) - 1))
# Allreduce algorithms to run every case through; the push two-shot needs the
# zero-copy mapping, so it joins in the zero-copy pass (Runner.ar_algos)
# "ll": LL up to its capacity (MPIGX_LL_MAX), the default choice above it;
# "ll2": the LL two-shot where a chunk fits half an LL slot;
# "oneshot"/"twoshot" force the staged algorithms
# "pull_generic": the zero-copy pull two-shot through the all-modes fold
# kernel instead of its dedicated kernel (ar_zc_kernel)
STAGED_ALGOS = ("ll", "ll2", "oneshot", "twoshot")
ZC_ALGOS = STAGED_ALGOS + ("push", "pull_generic", "pullpush")
ZC_ENV = {"MPIGX_ZC_MIN": "1", "MPIGX_ZC_REQUIRE": "1"}


# device buffers made for the current call: P(dev(x)) hands out a raw
# pointer, so the tensor must outlive the call (a freed block goes back to
# torch's cache, and the next allocation may take it before the engine reads
# it); Runner.run clears the list when the next call starts
_KEEP = []


def dev(a):
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    t = torch.empty(max(raw.size, 1) + 64, dtype=torch.uint8, device="cuda")[: raw.size]
    t.copy_(torch.from_numpy(raw.copy()))
    _KEEP.append(t)
    return t


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def host(t, dt):
    return t.cpu().numpy().view(dt)


class Runner:
    def __init__(self, comm, zc=False):
        """zc: comm was created with MPIGX_ZC_MIN set (the zero-copy pass)."""
        self.comm = comm
        self.zc = zc
        self.ar_algos = ZC_ALGOS if zc else STAGED_ALGOS
        self.L = MPI.lib()
        self.r = MPI.Comm_rank(comm)
        self.n = MPI.Comm_size(comm)
        self.fail = []
        self.ran = 0

    def knob(self, name, value):
        """Collective knob change (every rank, same value): mpigx_comm_set_knob."""
        MPI.set_knob(self.comm, name, value)

    def check(self, ok, what):
        self.ran += 1
        if not ok:
            self.fail.append(what)

    def run(self, coll, ins, dtname, opname, count, root=0, inplace=False):
        """Run one collective on my input ins[r]; return my output (numpy) or None."""
        L, r, n, cv = self.L, self.r, self.n, self.comm.val
        _KEEP.clear()
        npdt = M.DTYPES[dtname][1]
        h = M.DTYPES[dtname][0]
        op = M.OPS.get(opname, 0) if opname else 0
        x = ins[r]
        if coll in ("allreduce", "scan", "exscan"):
            recv = dev(x) if inplace else dev(np.full(x.size * x.itemsize, 0xCD, np.uint8))
            send = IN_PLACE if inplace else P(dev(x))
            f = {"allreduce": L.mpigx_allreduce, "scan": L.mpigx_scan, "exscan": L.mpigx_exscan}[coll]
            rc = f(send, P(recv), count, h, op, cv)
            assert rc == 0, (coll, rc)
            return host(recv, npdt)
        if coll == "reduce":
            isroot = r == root
            if inplace and isroot:
                recv = dev(x)
                rc = L.mpigx_reduce(IN_PLACE, P(recv), count, h, op, root, cv)
            else:
                recv = dev(np.zeros_like(x)) if isroot else None
                rc = L.mpigx_reduce(P(dev(x)), P(recv), count, h, op, root, cv)
            assert rc == 0, (coll, rc)
            return host(recv, npdt) if isroot else None
        if coll == "bcast":
            buf = dev(x)
            rc = L.mpigx_bcast(P(buf), count, h, root, cv)
            assert rc == 0
            return host(buf, npdt)
        if coll == "allgather":
            if inplace:
                full = np.zeros(count * n, dtype=npdt)
                full[r * count:(r + 1) * count] = x
                recv = dev(full)
                rc = L.mpigx_allgather(IN_PLACE, 0, 0, P(recv), count, h, cv)
            else:
                recv = dev(np.zeros(count * n, dtype=npdt))
                rc = L.mpigx_allgather(P(dev(x)), count, h, P(recv), count, h, cv)
            assert rc == 0
            return host(recv, npdt)
        if coll == "alltoall":
            if inplace:
                recv = dev(x)
                rc = L.mpigx_alltoall(IN_PLACE, 0, 0, P(recv), count, h, cv)
            else:
                recv = dev(np.zeros(count * n, dtype=npdt))
                rc = L.mpigx_alltoall(P(dev(x)), count, h, P(recv), count, h, cv)
            assert rc == 0
            return host(recv, npdt)
        raise KeyError(coll)

    def golden(self):
        cases, arr = load()
        for c in cases:
            if c["n"] != self.n or c["coll"] in ("reduce_local", "gather", "gatherv", "scatter", "scatterv",
                                                 "allgatherv", "alltoallv"):
                continue
            npdt = M.DTYPES[c["dtype"]][1]
            ins = typed(arr[c["id"] + ".in"], npdt)
            outs = typed(arr[c["id"] + ".out"], npdt)
            coll = c["coll"]
            algos = self.ar_algos if coll in ("allreduce", "reduce") else ("auto",)
            for algo in algos:
                self.knob("ALGO", algo)
                for inplace in (False, True):
                    if inplace and coll in ("bcast",):
                        continue
                    got = self.run(coll, ins, c["dtype"], c["op"], c["count"], c["root"], inplace)
                    exp = outs[self.r]
                    if coll == "reduce" and self.r != c["root"]:
                        continue
                    if coll == "exscan" and self.r == 0:
                        if not inplace:  # untouched 0xCD sentinel, like MPICH
                            self.check(np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (c["id"], algo, "rank0"))
                        continue
                    self.check(same_bits(got, exp), (c["id"], coll, c["dtype"], c["op"], algo, inplace))
        self.knob("ALGO", None)

    def vgolden(self):
        """Gather(v)/Scatter(v)/Allgatherv/Alltoallv golden cases (MPICH) through the C ABI,
        regular and IN_PLACE forms; the bytes past the result must stay untouched."""
        from test_oracle_golden import v_expected
        cases, arr = load()
        L, r, n, cv = self.L, self.r, self.n, self.comm.val
        I = ctypes.c_int * 16
        for c in cases:
            if c["n"] != n or "counts" not in c:
                continue
            npdt = M.DTYPES[c["dtype"]][1]
            h = M.DTYPES[c["dtype"]][0]
            es = np.dtype(npdt).itemsize
            ins = typed(arr[c["id"] + ".in"], npdt)
            seed, base, root, coll = c["seed"], c["count"], c["root"], c["coll"]
            K = [[M.vcnt(seed, a, b, base) for b in range(16)] for a in range(16)]
            exp = v_expected(c, ins).get(r)
            for inplace in (False, True):
                outn = (exp.size if exp is not None else 0) + 8
                recv = dev(np.full(outn * es, 0xCD, np.uint8))
                x = ins[r]
                if coll == "gather":
                    if inplace and r == root:
                        full = np.full(outn * es, 0xCD, np.uint8)
                        full[r * base * es:(r + 1) * base * es] = x[:base].view(np.uint8)
                        recv = dev(full)
                        rc = L.mpigx_gather(IN_PLACE, 0, 0, P(recv), base, h, root, cv)
                    else:
                        rc = L.mpigx_gather(P(dev(x[:base])), base, h, P(recv), base, h, root, cv)
                elif coll == "gatherv":
                    cnts = [K[p][0] for p in range(n)]
                    ds = [sum(cnts[:p]) for p in range(n)]
                    if inplace and r == root:
                        full = np.full(outn * es, 0xCD, np.uint8)
                        full[ds[r] * es:(ds[r] + cnts[r]) * es] = x[:cnts[r]].view(np.uint8)
                        recv = dev(full)
                        rc = L.mpigx_gatherv(IN_PLACE, 0, 0, P(recv), I(*cnts), I(*ds), h, root, cv)
                    else:
                        rc = L.mpigx_gatherv(P(dev(x[:cnts[r]])), cnts[r], h, P(recv), I(*cnts), I(*ds), h, root, cv)
                elif coll in ("scatter", "scatterv"):
                    cnts = [base] * n if coll == "scatter" else [K[p][1] for p in range(n)]
                    ds = [sum(cnts[:p]) for p in range(n)]
                    sb = P(dev(x)) if r == root else None
                    if inplace and r == root:
                        rc = (L.mpigx_scatter(sb, base, h, IN_PLACE, 0, 0, root, cv) if coll == "scatter" else
                              L.mpigx_scatterv(sb, I(*cnts), I(*ds), h, IN_PLACE, 0, 0, root, cv))
                        exp_r = None
                    else:
                        rc = (L.mpigx_scatter(sb, base, h, P(recv), base, h, root, cv) if coll == "scatter" else
                              L.mpigx_scatterv(sb, I(*cnts), I(*ds), h, P(recv), cnts[r], h, root, cv))
                elif coll == "allgatherv":
                    cnts = [K[p][2] for p in range(n)]
                    ds = [sum(cnts[:p]) for p in range(n)]
                    if inplace:
                        full = np.full(outn * es, 0xCD, np.uint8)
                        full[ds[r] * es:(ds[r] + cnts[r]) * es] = x[:cnts[r]].view(np.uint8)
                        recv = dev(full)
                        rc = L.mpigx_allgatherv(IN_PLACE, 0, 0, P(recv), I(*cnts), I(*ds), h, cv)
                    else:
                        rc = L.mpigx_allgatherv(P(dev(x[:cnts[r]])), cnts[r], h, P(recv), I(*cnts), I(*ds), h, cv)
                else:  # alltoallv
                    S = [[K[p][q] for q in range(n)] for p in range(n)]
                    sc = S[r]
                    sd = [sum(sc[:q]) for q in range(n)]
                    rcn = [S[p][r] for p in range(n)]
                    rd = [sum(rcn[:p]) for p in range(n)]
                    if inplace:
                        continue  # in-place alltoallv needs send layout == recv layout; covered below
                    rc = L.mpigx_alltoallv(P(dev(x[:sum(sc)])), I(*sc), I(*sd), h, P(recv), I(*rcn), I(*rd), h, cv)
                self.check(rc == 0, (c["id"], coll, "rc", rc))
                if exp is None or (coll in ("scatter", "scatterv") and inplace and r == root):
                    continue
                got = host(recv, np.uint8)
                ok = np.array_equal(got[:exp.nbytes], exp.view(np.uint8)) and (got[exp.nbytes:] == 0xCD).all()
                self.check(ok, (c["id"], coll, r, "inplace" if inplace else ""))
        # in-place alltoallv with a symmetric layout (recvcounts define the send layout too)
        cnt = [(p * 3 + r) % 4 + 1 for p in range(n)]  # rank r sends cnt[q] to q; symmetric needs S[p][r] == S[r][p]
        S = [[(p * 3 + q) % 4 + 1 + (q * 3 + p) % 4 for q in range(n)] for p in range(n)]
        sym = [[S[p][q] + S[q][p] for q in range(n)] for p in range(n)]
        ins = [np.arange(sum(sym[p]), dtype=np.float32) + 1000 * p for p in range(n)]
        rcn = [sym[p][r] for p in range(n)]
        rd = [sum(rcn[:p]) for p in range(n)]
        buf = dev(ins[r])
        rc = L.mpigx_alltoallv(IN_PLACE, None, None, 0, P(buf), I(*rcn), I(*rd), M.DTYPES["FLOAT"][0], cv)
        self.check(rc == 0, "alltoallv inplace rc")
        self.check(same_bits(host(buf, np.float32), M.alltoallv(ins, sym)[r]), "alltoallv inplace")
        del cnt

    def oracle_cases(self, sizes):
        """Larger seeded cases vs the (MPICH-pinned) oracle."""
        n, r = self.n, self.r
        for i, (dtname, opname, count) in enumerate(sizes):
            ins = make(dtname, opname, n, count, 1000 + i, edge=opname in ("MAX", "MIN"))
            for algo in self.ar_algos:
                self.knob("ALGO", algo)
                got = self.run("allreduce", ins, dtname, opname, count)
                self.check(same_bits(got, M.allreduce(ins, dtname, opname)[r], dtname == "BFLOAT16"), ("oracle-allreduce", dtname, opname, count, algo))
                root = (i + 1) % n
                got = self.run("reduce", ins, dtname, opname, count, root=root)
                if r == root:
                    self.check(same_bits(got, M.reduce(ins, dtname, opname, root), dtname == "BFLOAT16"), ("oracle-reduce", dtname, opname, count, algo))
            self.knob("ALGO", None)
            got = self.run("scan", ins, dtname, opname, count)
            self.check(same_bits(got, M.scan(ins, dtname, opname)[r], dtname == "BFLOAT16"), ("oracle-scan", dtname, opname, count))
            got = self.run("exscan", ins, dtname, opname, count)
            if r > 0:
                self.check(same_bits(got, M.exscan(ins, dtname, opname)[r], dtname == "BFLOAT16"), ("oracle-exscan", dtname, opname, count))
        # byte movers at sizes that span several blocks
        for count in (1, 4097, 300001):
            ins = make("FLOAT", "SUM", n, count * n, 77 + count)
            got = self.run("alltoall", ins, "FLOAT", None, count)
            self.check(same_bits(got, M.alltoall(ins, count)[r]), ("alltoall", count))
            ins1 = [x[:count] for x in ins]
            got = self.run("allgather", ins1, "FLOAT", None, count)
            self.check(same_bits(got, M.allgather(ins1)[r]), ("allgather", count))
            for algo in ("direct", "sag", "relay"):  # root pull vs scatter+allgather vs relay (zero-copy)
                self.knob("BCAST", algo)
                for root in sorted({0, n // 2, n - 1}):
                    got = self.run("bcast", ins1, "FLOAT", None, count, root=root)
                    self.check(same_bits(got, ins1[root]), ("bcast", algo, root, count))
            self.knob("BCAST", None)
        # bytes that are not a multiple of 16 per chunk, default algorithm choice
        for count in (262_145, 1_000_003):
            ins1 = make("UINT8_T", "BXOR", n, count, 91 + count)
            got = self.run("bcast", ins1, "UINT8_T", None, count, root=1 % n)
            self.check(same_bits(got, ins1[1 % n]), ("bcast-u8", count))

    def ll_cases(self):
        """M_AR_LL (small Allreduce, default up to MPIGX_LL_MAX = 64 KiB):
        byte counts around the 8-byte line and the 64 KiB limit, unaligned
        send buffers, IN_PLACE, and a stream-ordered burst of back-to-back
        LL launches (both area parities reused while peers run ahead) with
        other collectives between them; vs the MPICH-pinned oracle."""
        L, n, r, cv = self.L, self.n, self.r, self.comm.val
        self.knob("ALGO", "ll")  # LL up to the area's capacity (default: MPIGX_LL_AUTO)
        cases = (("UINT8_T", "BXOR", 1), ("UINT8_T", "SUM", 7), ("INT16_T", "MAX", 5), ("FLOAT", "SUM", 2),
                 ("FLOAT", "SUM", 3), ("DOUBLE", "PROD", 9), ("C_FLOAT_COMPLEX", "PROD", 17),
                 ("BFLOAT16", "SUM", 4099), ("INT64_T", "BAND", 1023), ("FLOAT", "MIN", 16384),
                 ("FLOAT", "SUM", 16385), ("UINT8_T", "BOR", 65537), ("DOUBLE", "SUM", 32768),
                 ("UINT8_T", "BOR", 262144), ("UINT8_T", "BOR", 262145))
        for i, (dt, op, count) in enumerate(cases):
            ins = make(dt, op, n, count, 4000 + i, edge=op in ("MAX", "MIN"))
            exp = M.allreduce(ins, dt, op)[r]
            for inplace in (False, True):
                got = self.run("allreduce", ins, dt, op, count, inplace=inplace)
                self.check(same_bits(got, exp, dt == "BFLOAT16"), ("ll", dt, op, count, inplace))
        # byte movers (C_BCAST_LL / C_ALLGATHER_LL / C_ALLTOALL_LL): ragged byte
        # counts (partial last line), the 64 KiB limit, every root, IN_PLACE
        for count in (1, 7, 13, 4097, 65537, 262144, 262145):
            ins = make("UINT8_T", "BXOR", n, count * n, 4300 + count)
            ins1 = [x[:count] for x in ins]
            for root in sorted({0, n // 2, n - 1}):
                got = self.run("bcast", ins1, "UINT8_T", None, count, root=root)
                self.check(same_bits(got, ins1[root]), ("ll-bcast", root, count))
            for inplace in (False, True):
                got = self.run("allgather", ins1, "UINT8_T", None, count, inplace=inplace)
                self.check(same_bits(got, M.allgather(ins1)[r]), ("ll-allgather", count, inplace))
                got = self.run("alltoall", ins, "UINT8_T", None, count, inplace=inplace)
                self.check(same_bits(got, M.alltoall(ins, count)[r]), ("ll-alltoall", count, inplace))
        # send buffer at an odd address (byte lines read bytewise)
        ins = make("UINT8_T", "SUM", n, 1001, 4100)
        raw = dev(np.concatenate([np.zeros(1, np.uint8), ins[r]]))
        recv = dev(np.zeros(1001, np.uint8))
        assert L.mpigx_allreduce(ctypes.c_void_p(raw.data_ptr() + 1), P(recv), 1001, M.DTYPES["UINT8_T"][0],
                                 M.OPS["SUM"], cv) == 0
        self.check(same_bits(host(recv, np.uint8), M.allreduce(ins, "UINT8_T", "SUM")[r]), "ll-odd-address")
        # stream-ordered burst: 40 LL launches (sizes vary, so grids vary) and a
        # Bcast every 7th, no host wait in between
        burst, outs = [], []
        for k in range(40):
            count = (1, 33, 4096, 16384)[k % 4] + k
            ins = make("FLOAT", "SUM", n, count, 4200 + k)
            burst.append((ins, count, dev(ins[r]), dev(np.zeros(count * 4, np.uint8))))
        bc = dev(np.full(64, r, np.uint8))
        L.mpigx_comm_set_blocking(cv, 0)
        for k, (ins, count, s, d) in enumerate(burst):
            assert L.mpigx_allreduce(P(s), P(d), count, M.DTYPES["FLOAT"][0], M.OPS["SUM"], cv) == 0
            if k % 7 == 6:
                assert L.mpigx_bcast(P(bc), 64, M.DTYPES["UINT8_T"][0], k % n, cv) == 0
        assert L.mpigx_comm_synchronize(cv) == 0
        L.mpigx_comm_set_blocking(cv, 1)
        for k, (ins, count, s, d) in enumerate(burst):
            self.check(same_bits(host(d, np.float32), M.allreduce(ins, "FLOAT", "SUM")[r]), ("ll-burst", k, count))
        if self.zc:
            # LL launches (12 KB IN_PLACE Scans, below a 16 KiB zero-copy
            # threshold) back to back with push two-shots (20 KB Allreduces,
            # above it), whose remote stores into the peers' arenas come before
            # any barrier: the host inserts one after an LL launch (mpigx.cpp
            # allreduce_push)
            zc_min = MPI.get_knob(self.comm, "ZC_MIN")
            self.knob("ZC_MIN", 16384)
            self.knob("ALGO", "push")
            pairs = []
            for k in range(12):
                a = make("INT32_T", "SUM", n, 3000 + k, 4400 + k)
                b = make("FLOAT", "SUM", n, 5000 + 7 * k, 4500 + k)
                pairs.append((a, b, dev(a[r]), dev(b[r]), dev(np.zeros((5000 + 7 * k) * 4, np.uint8))))
            L.mpigx_comm_set_blocking(cv, 0)
            for a, b, sa, sb, db in pairs:
                assert L.mpigx_scan(IN_PLACE, P(sa), a[r].size, M.DTYPES["INT32_T"][0], M.OPS["SUM"], cv) == 0
                assert L.mpigx_allreduce(P(sb), P(db), b[r].size, M.DTYPES["FLOAT"][0], M.OPS["SUM"], cv) == 0
            assert L.mpigx_comm_synchronize(cv) == 0
            L.mpigx_comm_set_blocking(cv, 1)
            self.knob("ALGO", None)
            self.knob("ZC_MIN", zc_min)
            for k, (a, b, sa, sb, db) in enumerate(pairs):
                self.check(same_bits(host(sa, np.int32), M.scan(a, "INT32_T", "SUM")[r]), ("ll-push-scan", k))
                self.check(same_bits(host(db, np.float32), M.allreduce(b, "FLOAT", "SUM")[r]), ("ll-push-ar", k))
        self.knob("ALGO", None)
        # the first Bcast (k = 6) spreads root 6 % n's value; later ones re-send it
        self.check(bool((host(bc, np.uint8) == 6 % n).all()), "ll-burst-bcast")

    def tune_cases(self):
        """The small/medium Allreduce tuner (no MPIGX_ALGO): the first calls of
        a size class run every candidate (LL / one-shot / two-shot) twice,
        then the class keeps one; every call must give MPICH's bits."""
        L, n, r, cv = self.L, self.n, self.r, self.comm.val
        self.knob("ALGO", None)
        for k, count in ((12, 1100), (13, 2500), (16, 20000), (18, 70000)):  # FLOAT: 4.4 KB .. 280 KB
            assert (count * 4).bit_length() - 1 == k
            for i in range(10):
                ins = make("FLOAT", "SUM", n, count + i, 4600 + 10 * k + i)
                got = self.run("allreduce", ins, "FLOAT", "SUM", count + i, inplace=bool(i % 2))
                self.check(same_bits(got, M.allreduce(ins, "FLOAT", "SUM")[r]), ("tune", k, i))
            ch = ctypes.c_int(-2)
            ns = (ctypes.c_double * 4)()
            assert L.mpigx_comm_tune_class(cv, k, ctypes.byref(ch), ns) == 0
            self.check(ch.value in (0, 1, 2, 3), ("tune-decided", k, ch.value))
        # the byte movers (kind 1-3: LL vs staged copy), 6 calls per class
        for k, count in ((11, 3000), (14, 20000)):  # UINT8 blocks: 3 KB, 20 KB
            for i in range(6):
                ins = make("UINT8_T", "BXOR", n, (count + i) * n, 4700 + 10 * k + i)
                ins1 = [x[:count + i] for x in ins]
                got = self.run("bcast", ins1, "UINT8_T", None, count + i, root=i % n)
                self.check(same_bits(got, ins1[i % n]), ("tune-bcast", k, i))
                got = self.run("allgather", ins1, "UINT8_T", None, count + i, inplace=bool(i % 2))
                self.check(same_bits(got, M.allgather(ins1)[r]), ("tune-allgather", k, i))
                got = self.run("alltoall", ins, "UINT8_T", None, count + i, inplace=bool(i % 2))
                self.check(same_bits(got, M.alltoall(ins, count + i)[r]), ("tune-alltoall", k, i))
            for kind in (1, 2, 3):
                ch = ctypes.c_int(-2)
                assert L.mpigx_comm_tune_class(cv, k + 64 * kind, ctypes.byref(ch), None) == 0
                self.check(ch.value in (0, 1), ("tune-decided-copy", kind, k, ch.value))

    def unaligned_cases(self):
        """Zero-copy Allreduce / Reduce on buffers 4 B past a 16-B boundary
        (the dedicated kernels' scalar paths; the kernel choice never looks
        at the pointers), every algorithm, IN_PLACE too, vs the oracle."""
        L, n, r, cv = self.L, self.n, self.r, self.comm.val
        count = 100_003
        ins = make("FLOAT", "SUM", n, count, 4700)
        exp = M.allreduce(ins, "FLOAT", "SUM")[r]
        h, op = M.DTYPES["FLOAT"][0], M.OPS["SUM"]
        for algo in ("pull", "pullpush", "pull_generic", "push", None):
            self.knob("ALGO", algo)
            for inplace in (False, True):
                sraw = dev(np.concatenate([np.zeros(1, np.float32), ins[r]]))
                rraw = dev(np.zeros(count + 1, np.float32)) if not inplace else sraw
                s = ctypes.c_void_p(sraw.data_ptr() + 4)
                d = ctypes.c_void_p(rraw.data_ptr() + 4)
                rc = L.mpigx_allreduce(IN_PLACE if inplace else s, d, count, h, op, cv)
                self.check(rc == 0, ("unaligned allreduce rc", algo, inplace))
                got = host(rraw, np.float32)[1:]
                self.check(same_bits(got, exp), ("unaligned allreduce", algo, inplace))
            root = (n - 1) if algo else 0
            sraw = dev(np.concatenate([np.zeros(1, np.float32), ins[r]]))
            rraw = dev(np.zeros(count + 1, np.float32))
            rc = L.mpigx_reduce(ctypes.c_void_p(sraw.data_ptr() + 4), ctypes.c_void_p(rraw.data_ptr() + 4), count, h,
                                op, root, cv)
            self.check(rc == 0, ("unaligned reduce rc", algo))
            if r == root:
                self.check(same_bits(host(rraw, np.float32)[1:], M.reduce(ins, "FLOAT", "SUM", root)),
                           ("unaligned reduce", algo))
        self.knob("ALGO", None)
        # Scan / Exscan (zero-copy pull-push at n <= 8: element path when a
        # buffer is off a 16-B boundary, vector path otherwise), in place too
        ins = make("INT32_T", "MAX", n, count, 4701, edge=True)
        hi = M.DTYPES["INT32_T"][0]
        for coll, fn, ref in (("scan", L.mpigx_scan, M.scan(ins, "INT32_T", "MAX")),
                              ("exscan", L.mpigx_exscan, M.exscan(ins, "INT32_T", "MAX"))):
            for off, inplace in ((4, False), (4, True), (0, True)):
                sraw = dev(np.concatenate([np.full(1, -7, np.int32), ins[r]]))
                rraw = dev(np.full(count + 1, -7, np.int32)) if not inplace else sraw
                s = ctypes.c_void_p(sraw.data_ptr() + off)
                d = ctypes.c_void_p(rraw.data_ptr() + off)
                if off == 0:  # aligned: the sentinel word goes to the end
                    sraw = dev(np.concatenate([ins[r], np.full(1, -7, np.int32)]))
                    rraw = sraw
                    s = d = P(sraw)
                rc = fn(IN_PLACE if inplace else s, d, count, hi, M.OPS["MAX"], cv)
                self.check(rc == 0, ("unaligned", coll, off, inplace, "rc", rc))
                got = host(rraw, np.int32)
                body, sent = (got[1:], got[0]) if off else (got[:-1], got[-1])
                exp = ref[r] if not (coll == "exscan" and r == 0) else (ins[0] if inplace else np.full(count, -7, np.int32))
                self.check(same_bits(body, exp) and sent == -7, ("unaligned", coll, off, inplace))

    def ring_cases(self, nchs=(1, 2, 4)):
        """MPIGX_ALGO=ring (zero-copy path): bit-exact against the ring's own
        association (oracle fold_ring, rounds included), and against MPICH:
        integer / bitwise ops exact, float SUM within the stated tolerance
        2(n-1) u sum|x| (oracle sum_tolerance)."""
        n, r = self.n, self.r
        stage = MPI.get_knob(self.comm, "STAGING_BYTES")
        cases = (("FLOAT", "SUM", 1_000_003), ("DOUBLE", "SUM", 65537), ("FLOAT", "MAX", 100_001),
                 ("INT32_T", "BAND", 262_147), ("INT64_T", "SUM", 50_000), ("BFLOAT16", "SUM", 40_000),
                 ("C_FLOAT_COMPLEX", "PROD", 3333), ("UINT8_T", "BXOR", 100_000), ("FLOAT", "SUM", 5))
        self.knob("ALGO", "ring")
        for nch in nchs:
            self.knob("RING_CHANNELS", nch)
            for i, (dt, op, count) in enumerate(cases):
                ins = make(dt, op, n, count, 3000 + i, edge=op in ("MAX", "MIN"))
                exp = M.fold_ring(ins, dt, op, nch, M.ring_round_elems(stage, n, dt, nch))
                for inplace in (False, True):
                    got = self.run("allreduce", ins, dt, op, count, inplace=inplace)
                    self.check(same_bits(got, exp, dt == "BFLOAT16"), ("ring", nch, dt, op, count, inplace))
                kind = M.DTYPES[dt][2]
                mp = M.allreduce(ins, dt, op)[0]
                if kind in ("int", "uint", "byte"):
                    self.check(np.array_equal(exp, mp), ("ring-vs-mpich", dt, op))
                elif dt in ("FLOAT", "DOUBLE") and op == "SUM":
                    err = np.abs(exp.astype(np.float64) - mp.astype(np.float64))
                    self.check(bool((err <= M.sum_tolerance(ins, dt)).all()), ("ring-tolerance", dt, count))
        self.knob("ALGO", None)
        self.knob("RING_CHANNELS", 1)

    def linear_order(self):
        MPI.set_reduce_order(self.comm, 1)
        for i, (dtname, opname, count) in enumerate((("FLOAT", "SUM", 5000), ("DOUBLE", "SUM", 70001),
                                                    ("FLOAT", "MAX", 3000), ("BFLOAT16", "SUM", 9999))):
            ins = make(dtname, opname, self.n, count, 500 + i, edge=opname == "MAX")
            for algo in self.ar_algos:
                self.knob("ALGO", algo)
                got = self.run("allreduce", ins, dtname, opname, count)
                self.check(same_bits(got, M.fold_linear(ins, dtname, opname), dtname == "BFLOAT16"), ("linear", dtname, opname, algo))
        self.knob("ALGO", None)
        MPI.set_reduce_order(self.comm, 0)

    def errors(self):
        L, cv = self.L, self.comm.val
        t = dev(np.zeros(16, np.float32))
        self.check(L.mpigx_allreduce(P(t), P(t), 4, M.DTYPES["FLOAT"][0], M.OPS["BAND"], cv) == 9, "err-op")
        self.check(L.mpigx_allreduce(P(t), P(t), 4, 42, M.OPS["SUM"], cv) == 3, "err-type")
        self.check(L.mpigx_allreduce(P(t), P(t), -1, M.DTYPES["FLOAT"][0], M.OPS["SUM"], cv) == 2, "err-count")
        self.check(L.mpigx_reduce(P(t), P(t), 4, M.DTYPES["FLOAT"][0], M.OPS["SUM"], self.n, cv) == 7, "err-root")
        self.check(L.mpigx_bcast(P(t), 4, M.DTYPES["FLOAT"][0], -1, cv) == 7, "err-root-bcast")
        self.check(L.mpigx_allreduce(None, None, 0, M.DTYPES["FLOAT"][0], M.OPS["SUM"], cv) == 0, "count0")


def run_pass(name, comm, zc, phase):
    """Every phase of one pass on comm; returns the pass's summary."""
    R = Runner(comm, zc)
    if phase != "oracle":  # MPICH-recorded cases exist for n <= 8
        R.golden()
        R.vgolden()
    R.errors()
    R.ll_cases()
    if not zc:
        R.tune_cases()
    R.oracle_cases([("FLOAT", "SUM", 1_000_003), ("DOUBLE", "SUM", 65537), ("FLOAT", "MAX", 100_001),
                    ("INT32_T", "BAND", 262_147), ("INT64_T", "MAX", 50_000), ("BFLOAT16", "SUM", 40_000),
                    ("C_FLOAT_COMPLEX", "PROD", 3333), ("UINT8_T", "BXOR", 100_000)])
    R.linear_order()
    if zc:
        R.ring_cases()
        R.unaligned_cases()
    if phase == "all":
        # rounds: a communicator whose staging arena is 1 MiB forces multi-round launches
        stage = os.environ.get("MPIGX_STAGING_BYTES")
        os.environ["MPIGX_STAGING_BYTES"] = str(1 << 20)
        c2 = MPI.Comm_dup(comm)
        if stage is None:  # the next pass's communicator gets the launch's arena again
            del os.environ["MPIGX_STAGING_BYTES"]
        else:
            os.environ["MPIGX_STAGING_BYTES"] = stage
        assert MPI.get_knob(c2, "STAGING_BYTES") == 1 << 20
        R2 = Runner(c2, zc)
        R2.oracle_cases([("FLOAT", "SUM", 700_001), ("DOUBLE", "MIN", 300_001)])
        if zc:
            R2.ring_cases(nchs=(1, 2))
        MPI.free(c2)
        R.fail += R2.fail
        R.ran += R2.ran
    MPI.Barrier(comm)
    pm = list(MPI.peer_memory(comm))  # signalling protocol per peer pair (rw_mask, same_device)
    summary = {"pass": name, "rank": R.r, "n": R.n, "peer_mem": pm, "checks": R.ran,
               "failures": [str(f) for f in R.fail[:20]], "nfail": len(R.fail)}
    if zc:  # launches on an agreed zero-copy view: buffer exchanges, and hits on an earlier exchange's view
        hits, exch = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        assert R.L.mpigx_comm_zc_stats(comm.val, ctypes.byref(hits), ctypes.byref(exch)) == 0
        summary.update(zc_exchanges=exch.value, zc_hits=hits.value)
    return summary


def main():
    world = MPI.Init()
    phase = os.environ.get("MPIGX_TEST_PHASE", "all")
    world_zc = bool(os.environ.get("MPIGX_ZC_MIN"))
    passes = os.environ.get("GOLDEN_PASSES", "zc" if world_zc else "staged").split(",")
    assert passes and set(passes) <= {"staged", "zc"} and len(set(passes)) == len(passes), passes
    summaries = []
    for name in passes:
        zc = name == "zc"
        comm = world
        if zc != world_zc:
            assert zc, "a staged pass needs a launch without MPIGX_ZC_MIN"
            os.environ.update(ZC_ENV)  # every rank, before its part of the collective Comm_dup
            comm = MPI.Comm_dup(world)
            assert MPI.get_knob(comm, "ZC_MIN") == 1 and MPI.get_knob(comm, "ZC_REQUIRE") == 1
            assert MPI.get_knob(comm, "STAGING_BYTES") == MPI.get_knob(world, "STAGING_BYTES")
        summaries.append(run_pass(name, comm, zc, phase))
        if comm is not world:
            MPI.free(comm)
    MPI.Finalize()
    for s in summaries:
        print(json.dumps(s), flush=True)
    sys.exit(1 if any(s["nfail"] for s in summaries) else 0)


if __name__ == "__main__":
    main()
