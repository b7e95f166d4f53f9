"""Write-footprint harness of the collectives and the local fold (numpy only,
importable without a GPU): where bytes land, not what value they have.

Every buffer of a call is one uint8 allocation laid out as

    [ pre-guard 4 KiB | pad | payload | post-guard 64 KiB ]

with the payload `off` bytes past a 256-B boundary (the allocation itself is
256-B aligned; the worker asserts it).  Guards, pad and the initial content of
an out-of-place recvbuf hold a position-, rank- and salt-dependent byte
pattern, so a kernel that copies one guard over another, or stores zeros over
zeros, still changes bytes.  The post-guard is larger than the largest single
over-store in the kernels (the 16 KiB `U * kThreads * 16` output span of a
block) and than a slice at the sizes of the table.

`verify` compares a buffer read back after the call with its image: the
payload against the expected result (golden_io.same_bits), the first modified
byte of the pre-guard, the pad and the post-guard, and, for a buffer the call
may only read, any changed byte anywhere.

`send_off` / `recv_off` give every rank its own byte offsets, so the pointers a
zero-copy kernel sees (its own and its peers') mix 16-B aligned and misaligned
buffers; `cases(n)` is the deterministic table of calls, the same on every
rank; `expected(case, n)` runs it through the MPICH-pinned models.
"""
import numpy as np

from gen_inputs import make
from golden_io import same_bits
from oracle import mpich_model as M
import redscat_model as R

PRE, POST, ALIGN = 4096, 64 << 10, 256
KINDS = ("payload", "pre", "pad", "post", "readonly")

# knob defaults the applicability conditions below are stated against
LL_MAX = 256 << 10       # MPIGX_LL_MAX: capacity of one LL sender slot
STAGE = 64 << 20         # MPIGX_STAGING_BYTES of the ordinary launches
SMALL_STAGE = 4096       # the floor knobs_from_env / knob_apply clamp the arena to (one page)


def pattern(total, rank, salt):
    i = np.arange(total, dtype=np.int64)
    return ((131 * i + 17 * rank + salt) & 0xFF).astype(np.uint8)


class Guarded:
    """Host image of one guarded buffer.  payload: typed array to place, or
    None to leave the pattern there (`nbytes` of it)."""

    def __init__(self, payload, off, rank, salt, nbytes=None, readonly=False, expect=None, npdt=None, bf16=False):
        raw = None if payload is None else np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        nbytes = raw.size if raw is not None else int(nbytes)
        assert 0 <= off < ALIGN
        self.lo = PRE + off
        self.hi = self.lo + nbytes
        self.image = pattern(self.hi + POST, rank, salt)
        if raw is not None:
            self.image[self.lo:self.hi] = raw
        self.readonly = readonly
        self.expect = expect      # typed expected payload (None with readonly: the image itself)
        self.npdt = npdt
        self.bf16 = bf16

    @property
    def nbytes(self):
        return self.hi - self.lo


def _first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return int(d[0]) if d.size else -1


def verify(g, got):
    """Findings (dicts with "kind" in KINDS and byte offsets) of buffer `got`
    (uint8, read back after the call) against its image `g`."""
    got = np.asarray(got).view(np.uint8).reshape(-1)
    out = []
    if got.size != g.image.size:
        return [{"kind": "payload", "why": f"size {got.size} != {g.image.size}"}]
    if g.readonly:
        i = _first_diff(got, g.image)
        if i >= 0:
            region = "pre" if i < PRE else "pad" if i < g.lo else "payload" if i < g.hi else "post"
            out.append({"kind": "readonly", "offset": i, "region": region, "rel": i - g.lo})
        return out
    for kind, a, b in (("pre", 0, PRE), ("pad", PRE, g.lo), ("post", g.hi, got.size)):
        i = _first_diff(got[a:b], g.image[a:b])
        if i >= 0:
            out.append({"kind": kind, "offset": a + i, "rel": i, "nbad": int((got[a:b] != g.image[a:b]).sum())})
    if g.expect is not None:
        exp = np.ascontiguousarray(g.expect)
        have = got[g.lo:g.hi].copy().view(exp.dtype)
        if not same_bits(have, exp, bf16=g.bf16):
            es = exp.itemsize
            bad = -1
            if have.shape == exp.shape and exp.size:
                d = np.nonzero((have.view(np.uint8).reshape(-1, es) != exp.view(np.uint8).reshape(-1, es)).any(1))[0]
                bad = int(d[0]) if d.size else -1
            out.append({"kind": "payload", "first_bad_elem": bad, "elems": int(exp.size)})
    return out


# ---------------------------------------------------------------------------
# per-rank byte offsets, by the alignment unit `align` (1, 2, 4 or 8: comp_align)
# ---------------------------------------------------------------------------
# rank 0 aligned on both, rank 1 misaligned on send only (by 4: the 4-B branch
# of block_copy against an aligned peer), rank 2 on recv only (an odd multiple
# of the unit: the byte fallback for 1- and 2-byte types), the others mixed
_SEND = {1: (0, 4, 0, 2, 7, 0, 13, 8), 2: (0, 4, 0, 2, 14, 0, 6, 8), 4: (0, 4, 0, 8, 12, 0, 8, 12),
         8: (0, 8, 0, 0, 8, 8, 0, 8)}
_RECV = {1: (0, 0, 3, 4, 9, 12, 6, 1), 2: (0, 0, 6, 4, 10, 12, 2, 8), 4: (0, 0, 12, 4, 8, 4, 12, 8),
         8: (0, 0, 8, 8, 0, 8, 0, 8)}


def send_off(r, es, align):
    assert es % align == 0
    return _SEND[align][r % 8]


def recv_off(r, es, align):
    assert es % align == 0
    return _RECV[align][r % 8]


def comp_align(dt):
    """Alignment unit of a type's offsets: its size, the component size for a
    complex type (legal in MPI, what a numpy view gives; element-granular
    offsets never produce it)."""
    d = np.dtype(M.DTYPES[dt][1])
    return d.itemsize // 2 if d.kind == "c" else d.itemsize


# ---------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------
DTYPE_OPS = (("INT8_T", ("SUM", "MAX", "BAND")), ("INT16_T", ("MIN", "SUM", "BXOR")), ("BFLOAT16", ("SUM", "MAX")),
             ("FLOAT", ("SUM", "MIN", "PROD")), ("DOUBLE", ("MAX", "SUM")), ("C_DOUBLE_COMPLEX", ("SUM", "PROD")))
INT_TYPES = ("INT8_T", "INT16_T")
REDUCING = ("allreduce", "reduce", "reduce_scatter_block", "reduce_scatter")
MOVING = ("bcast", "allgather", "alltoall")
SCANS = ("scan", "exscan")
FAMILY = {**{c: "reducing" for c in REDUCING}, **{c: "moving" for c in MOVING}, **{c: "scan" for c in SCANS}}
# the fuzz worker's ALGOS (tests/spmd/fuzz_worker.py), as (name, zero-copy)
AR_ALGOS = (("auto", 0), ("ll", 0), ("ll2", 0), ("oneshot", 0), ("twoshot", 0), ("push", 1), ("pull", 1),
            ("pull_generic", 1), ("pullpush", 1))


def esize(dt):
    return np.dtype(M.DTYPES[dt][1]).itemsize


def counts_for(dt, n):
    """1, W - 1, W + 1 (W = elements per 16-B vector), 2 n W + 1 (every chunk
    whole vectors, the last a ragged tail), 16 n W + 3 (16 blocks with a slice
    each, edges inside vectors), and one near 4099."""
    w = max(1, 16 // esize(dt))
    return (1, max(1, w - 1), w + 1, 2 * n * w + 1, 16 * n * w + 3, 4099)


def paths(n):
    """(collective, path, knobs, variants): knobs select the path
    (mpigx.cpp reduce_common / bcast_impl / gather_like / scan_common /
    reduce_scatter_common); ZC = 1 means ZC_MIN = 1 and ZC_REQUIRE = 1 (a
    fall-back to staging is then an error), ZC = 0 the default ZC_MIN (16 MiB:
    nothing here reaches it).  Every launch sets AR_TUNE = 0, so no tuner picks.
    variants: dicts merged into the case (root, inplace, v)."""
    P = []
    both = ({"inplace": False}, {"inplace": True})
    # Allreduce.  Without zero-copy and with ALGO auto / oneshot: the staged
    # one-shot (bytes <= ONESHOT_MAX = 256 KiB); twoshot: staged two-shot;
    # ll: ll_take, bytes <= LL_MAX and n * LL_MAX <= arena; ll2: ll2_fits,
    # chunk <= LL_MAX / 2 (ll_ok below restates both; the CPU test asserts
    # them).  With zero-copy the algorithm names pick the kernel: push
    # (M_AR_PUSH), pull (ar_zc_kernel AG_PULL), pull_generic (fold_kernel
    # M_AR_ZC), pullpush (ar_zc_kernel AG_PUSH, n <= 8), ring (ring_kernel).
    for a, zc in AR_ALGOS:
        P.append(("allreduce", a, {"ALGO": a, "ZC": zc}, both))
    P.append(("allreduce", "pullpush_slices3", {"ALGO": "pullpush", "ZC": 1, "AR_SLICES": 3}, both))
    for ch in (1, 2):  # integer types only: any association gives these bits
        P.append(("allreduce", f"ring{ch}", {"ALGO": "ring", "ZC": 1, "RING_CHANNELS": ch}, both))
    # MPIGX_ORDER_LINEAR: S_LINEAR has no dedicated kernel, the pull runs in fold_kernel
    P.append(("allreduce", "linear", {"ALGO": "pull", "ZC": 1, "LINEAR": 1}, both))
    # Reduce: staged one- and two-shot, the LL step (ALGO ll, as Allreduce),
    # zero-copy straight into the root's recvbuf (reduce_zc_push) and, with
    # pull_generic, through the arena (fold_kernel M_RED_ZC)
    roots = tuple({"root": q, "inplace": ip} for q, ip in ((0, False), (n - 1, True), (n - 1, False), (0, True)))
    for path, kn in (("oneshot", {"ALGO": "oneshot", "ZC": 0}), ("twoshot", {"ALGO": "twoshot", "ZC": 0}),
                     ("ll", {"ALGO": "ll", "ZC": 0}), ("zc", {"ALGO": "auto", "ZC": 1}),
                     ("zc_generic", {"ALGO": "pull_generic", "ZC": 1})):
        P.append(("reduce", path, kn, roots))
    # Bcast: MPIGX_BCAST names the algorithm (the LL step is then never taken);
    # staged, relay runs the scatter + allgather
    for mode in ("direct", "sag", "relay"):
        for zc in (0, 1):
            P.append(("bcast", f"{mode}_{'zc' if zc else 'staged'}", {"BCAST": mode, "ZC": zc},
                      ({"root": 0}, {"root": n - 1}, {"root": 1 % n})))
    # Allgather / Alltoall: ALGO auto, LL_AUTO = 0 keeps the LL step off.  The
    # zero-copy Alltoall is out of place only: IN_PLACE under the zero-copy
    # knobs runs the staged rounds (gather_like), and is listed as such
    for coll in ("allgather", "alltoall"):
        P.append((coll, "staged", {"ZC": 0}, both))
        P.append((coll, "zc", {"ZC": 1}, both if coll == "allgather" else ({"inplace": False},)))
    P.append(("alltoall", "zc_knobs_inplace_staged", {"ZC": 1}, ({"inplace": True},)))
    # Scan / Exscan: pull-push (SCAN_PP = 1, zero-copy, in place too), the
    # zero-copy pull (SCAN_PP = 0, out of place only: scan_common stages
    # IN_PLACE there), the staged rounds (LL_AUTO = 0: no LL step)
    for coll in SCANS:
        P.append((coll, "pp", {"ZC": 1, "SCAN_PP": 1}, both))
        P.append((coll, "pull", {"ZC": 1, "SCAN_PP": 0}, ({"inplace": False},)))
        P.append((coll, "staged", {"ZC": 0, "SCAN_PP": 1}, both))
    # Reduce_scatter_block / Reduce_scatter (n <= 8): staged (M_RS_PUSH) and zero-copy (M_RS_ZC)
    for coll in ("reduce_scatter_block", "reduce_scatter"):
        for zc in (0, 1):
            P.append((coll, "zc" if zc else "staged", {"ZC": zc}, both))
    return P


def _v_counts(count, n, j):
    """Receive counts of a v case: base + (q % 3) - 1, and rank (j % n) empty
    in every other case (a zero-count rank)."""
    c = [max(0, count + (q % 3) - 1) for q in range(n)]
    if j % 2 == 0:
        c[j % n] = 0
    return c


def cases(n, per_variant=3):
    """The table for world size n: every (collective, path, variant) gets
    `per_variant` cases; dtypes, ops and counts rotate through them, so every
    dtype meets every collective family and every count every dtype."""
    out = []
    j = 0
    for coll, path, knobs, variants in paths(n):
        ints = path.startswith("ring")
        for var in variants:
            for _ in range(per_variant):
                if ints:
                    dt = INT_TYPES[j % 2]
                    ops = dict(DTYPE_OPS)[dt]
                else:
                    dt, ops = DTYPE_OPS[j % len(DTYPE_OPS)]
                cs = counts_for(dt, n)
                count = cs[(j // len(DTYPE_OPS) + j) % len(cs)]
                c = {"id": j, "coll": coll, "path": path, "knobs": dict(knobs), "dtype": dt,
                     "op": None if coll in MOVING else ops[(j // 7) % len(ops)], "count": count, "root": 0,
                     "inplace": False, "seed": 4000 + j, "edge": j % 2 == 0}
                c.update(var)
                if coll == "reduce_scatter":
                    c["counts"] = _v_counts(count, n, j)
                elif coll == "reduce_scatter_block":
                    c["counts"] = [count] * n
                out.append(c)
                j += 1
    return out


def small_arena_cases(n):
    """The launch with the arena at its floor (SMALL_STAGE = 4096 B: one round
    of Allreduce / Reduce holds 4096 / es elements rounded down to n vectors,
    of Bcast 4096 B, of Reduce_scatter 4096 / n rounded down to 16 B per
    sender): messages of at least three rounds, so round boundaries are
    footprint edges.  The LL step needs n * LL_MAX <= arena and is never taken."""
    out = []
    j = 0
    specs = [("allreduce", "twoshot", {"ALGO": "twoshot", "ZC": 0}), ("allreduce", "oneshot", {"ALGO": "oneshot", "ZC": 0}),
             ("reduce", "twoshot", {"ALGO": "twoshot", "ZC": 0}), ("reduce", "oneshot", {"ALGO": "oneshot", "ZC": 0}),
             ("bcast", "direct_staged", {"BCAST": "direct", "ZC": 0}), ("bcast", "sag_staged", {"BCAST": "sag", "ZC": 0}),
             ("reduce_scatter_block", "staged", {"ZC": 0}), ("reduce_scatter", "staged", {"ZC": 0})]
    for coll, path, knobs in specs:
        for k in range(4):
            dt, ops = DTYPE_OPS[(j + k) % len(DTYPE_OPS)]
            es = esize(dt)
            per_round = SMALL_STAGE // es if coll not in REDUCING[2:] else SMALL_STAGE // n // es
            count = 3 * per_round + (5, 1, 16 // min(es, 16) + 1, 77)[k]  # >= 3 full rounds and a ragged one
            c = {"id": 10000 + j, "coll": coll, "path": path, "knobs": dict(knobs), "dtype": dt,
                 "op": None if coll in MOVING else ops[j % len(ops)], "count": count, "root": (0, n - 1)[k % 2],
                 "inplace": bool(k & 2) and coll != "bcast", "seed": 9000 + j, "edge": k % 2 == 0}
            if coll == "reduce_scatter":
                c["counts"] = _v_counts(count, n, j + 1)
            elif coll == "reduce_scatter_block":
                c["counts"] = [count] * n
            out.append(c)
            j += 1
    return out


def complex_cases(n):
    """Component-aligned complex buffers (C_DOUBLE_COMPLEX at byte offset 8,
    C_FLOAT_COMPLEX at 4 / 8 / 12: comp_align in the offset table) through the
    staged two-shot and the zero-copy pull Allreduce.  No pointer is then a
    multiple of the element size; the kernels take their scalar paths
    (`Vec<T, 1>` loads and stores of whole elements at component alignment)."""
    out = []
    j = 0
    for path, knobs in (("twoshot", {"ALGO": "twoshot", "ZC": 0}), ("pull", {"ALGO": "pull", "ZC": 1})):
        for dt in ("C_DOUBLE_COMPLEX", "C_FLOAT_COMPLEX"):
            for count in counts_for(dt, n)[2:]:
                out.append({"id": 20000 + j, "coll": "allreduce", "path": path, "knobs": dict(knobs), "dtype": dt,
                            "op": ("SUM", "PROD")[j % 2], "count": count, "root": 0, "inplace": j % 3 == 1,
                            "seed": 12000 + j, "edge": False})
                j += 1
    return out


def zc_calls(cs):
    """Calls of a table that launch a zero-copy kernel (each takes one buffer
    exchange or one hit of the optimistic view: mpigx_comm_zc_stats)."""
    return sum(1 for c in cs if c["knobs"].get("ZC") and not (c["coll"] == "alltoall" and c["inplace"]))


def rounds(c, n, stage=SMALL_STAGE):
    """Staging rounds of a staged case (mpigx.cpp: reduce_common `round`,
    bcast_impl `round`, reduce_scatter_common `round`)."""
    es = esize(c["dtype"])
    vec = max(1, 16 // es)
    if c["coll"] in ("allreduce", "reduce"):
        per = (stage // es) // (n * vec) * n * vec
        return -(-c["count"] // per)
    if c["coll"] == "bcast":
        return -(-(c["count"] * es) // (stage & ~15))
    per = (stage // n) // 16 * 16 // es // vec * vec
    return -(-max(c["counts"]) // per)


def ll_ok(c, n, ll_max=LL_MAX, stage=STAGE):
    """The forced LL paths' applicability (mpigx.cpp ll_take / ll2_fits):
    where it is False the call would silently run the staged kernels."""
    es = esize(c["dtype"])
    nbytes = c["count"] * es
    algo = c["knobs"].get("ALGO")
    if n * ll_max > stage:
        return False
    if algo == "ll":
        return nbytes <= ll_max
    if algo == "ll2":
        vec = max(1, 16 // es)
        chunk = -(-(-(-c["count"] // n)) // vec) * vec * es
        return n > 1 and chunk <= ll_max // 2
    return True


# ---------------------------------------------------------------------------
# inputs, expected values, buffers of one rank
# ---------------------------------------------------------------------------
def send_elems(c, n):
    if c["coll"] == "alltoall":
        return c["count"] * n
    if c["coll"] in ("reduce_scatter_block", "reduce_scatter"):
        return sum(c["counts"])
    return c["count"]


def recv_elems(c, n, r):
    if c["coll"] in ("allgather", "alltoall"):
        return c["count"] * n
    if c["coll"] in ("reduce_scatter_block", "reduce_scatter"):
        return c["counts"][r]
    return c["count"]


def inputs(c, n):
    return make(c["dtype"], c["op"] or "SUM", n, send_elems(c, n), c["seed"], edge=c["edge"])


def expected(c, n, ins=None):
    """Per-rank results (typed arrays; None where the call defines none: a
    Reduce non-root, Exscan's rank 0) from oracle/mpich_model.py and
    tests/redscat_model.py."""
    ins = inputs(c, n) if ins is None else ins
    coll, dt, op = c["coll"], c["dtype"], c["op"]
    if coll == "allreduce":
        if c["knobs"].get("LINEAR"):
            v = M.fold_linear(ins, dt, op)
            return [v] * n
        return M.allreduce(ins, dt, op)
    if coll == "reduce":
        v = M.reduce(ins, dt, op, c["root"])
        return [v if r == c["root"] else None for r in range(n)]
    if coll == "scan":
        return M.scan(ins, dt, op)
    if coll == "exscan":
        return M.exscan(ins, dt, op, untouched=None)
    if coll == "bcast":
        return M.bcast(ins, c["root"])
    if coll == "allgather":
        return M.allgather(ins)
    if coll == "alltoall":
        return M.alltoall(ins, c["count"])
    return R.reduce_scatter(ins, c["counts"], dt, op)


def buffers(c, n, r, ins, outs, align=None):
    """(send, recv) of rank r: Guarded images, send None where the call takes
    IN_PLACE (or has no sendbuf: Bcast).  A Reduce non-root gets a non-null
    recvbuf that must stay wholly unchanged, as Exscan's rank 0 and Bcast's
    root do; every sendbuf is read-only."""
    dt, coll = c["dtype"], c["coll"]
    npdt = np.dtype(M.DTYPES[dt][1])
    es = npdt.itemsize
    a = align or comp_align(dt)
    so, ro = send_off(r, es, a), recv_off(r, es, a)
    bf = dt == "BFLOAT16"
    salt = 7 * c["id"]
    x = ins[r]
    exp = outs[r]
    kw = {"npdt": npdt, "bf16": bf}
    sg = Guarded(x, so, r, salt + 1, readonly=True, **kw)
    nrecv = recv_elems(c, n, r) * es
    if coll == "bcast":
        if r == c["root"]:
            return None, Guarded(x, ro, r, salt, readonly=True, **kw)
        return None, Guarded(None, ro, r, salt, nbytes=nrecv, expect=exp, **kw)
    if coll == "reduce" and r != c["root"]:
        return sg, Guarded(None, ro, r, salt, nbytes=nrecv, readonly=True, **kw)
    if coll == "exscan" and r == 0:
        if c["inplace"]:
            return None, Guarded(x, ro, r, salt, readonly=True, **kw)
        return sg, Guarded(None, ro, r, salt, nbytes=nrecv, readonly=True, **kw)
    if not c["inplace"]:
        return sg, Guarded(None, ro, r, salt, nbytes=nrecv, expect=exp, **kw)
    if coll == "allgather":
        rg = Guarded(None, ro, r, salt, nbytes=nrecv, expect=exp, **kw)
        rg.image[rg.lo + r * x.nbytes: rg.lo + (r + 1) * x.nbytes] = x.view(np.uint8)
        return None, rg
    if coll in ("reduce_scatter_block", "reduce_scatter"):
        # the result takes the first counts[r] elements; the rest of the buffer is input and stays
        return None, Guarded(x, ro, r, salt, expect=np.concatenate([exp, x[exp.size:]]), **kw)
    return None, Guarded(x, ro, r, salt, expect=exp, **kw)
