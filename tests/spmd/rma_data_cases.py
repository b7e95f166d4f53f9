"""Case plan and model of the RMA data-path tests, shared by the CPU test of
the plan (tests/test_rma_data_cpu.py) and the GPU worker
(tests/spmd/rma_data_worker.py) so both see the same cases and values.

The semantic matrix (rma_cases.py) runs at 12 elements; this plan chooses
counts from the launch arithmetic of the three device paths instead:

* Accumulate / Get_accumulate / Fetch_and_op: acc_kernel (kernels.hpp) is
  launched by rma.cpp apply_one with g = clamp(ceil(count / 1024), 1, 1024)
  blocks of 256 threads, nt = 256 g, a 4-way unrolled grid-stride main loop
  (i + 3 nt < count) and a one-per-stride tail (`acc_geometry`).
* Get_accumulate goes through one scratch slot per origin in chunks of
  per = slot_bytes / esize elements (rma.cpp acc_common, `seam_per`).
* Put / Get: xfer_kernel (copy.hip) cuts the bytes into
  g = clamp(ceil(bytes / 64 Ki), 1, 256) slices rounded up to 16 B, each
  copied by block_copy (device.hpp), which takes a 16-B vector branch, a 4-B
  branch or a byte branch from (dst ^ src) and peels a head up to the
  destination's alignment (`copy_geometry`).

Rank r targets (r + 1) % n, so every window has one origin and the expected
window does not depend on arrival order.  Every case owns a range of its
type's window with GUARD sentinel elements on both sides; the expectation is
a model of the whole window (oracle/rma_model.py, pinned to MPICH by
rma_golden.json; bf16 through oracle/mpich_model.apply_op, parity unpinned).
"""
import numpy as np

from oracle import mpich_model as M
from oracle import rma_model as R

TYPES = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64",
         "complex64", "complex128", "bfloat16"]
OPS = ["SUM", "PROD", "MIN", "MAX", "LAND", "LOR", "LXOR", "BAND", "BOR", "BXOR", "REPLACE", "NO_OP"]
MPI_NAME = {"bfloat16": "BFLOAT16", **{np.dtype(k).name: v for k, v in R.NP_TO_MPI.items()}}
# one type of each element size for the capped counts and the chunk seams
SIZE_TYPES = ["int8", "bfloat16", "float32", "float64", "complex128"]

GUARD = 64          # sentinel elements (bytes in uint8 windows) around every range
SENTINEL = 0xCD     # byte pattern of guards: no NaN in any float type, not 0 / 1
RES_GUARD = 32      # guard bytes before and after a result / origin-side destination view

# acc_kernel launch geometry (rma.cpp apply_one, kernels.hpp acc_kernel)
ACC_THREADS, ACC_U, ACC_MAX_BLOCKS = 256, 4, 1024
MATRIX_COUNTS = [1024, 1025, 4099]
CAPPED_COUNTS = [1 << 20, (2 << 20) + 517]
SMALL_COUNTS = [1, 255]
ACC_COUNTS = SMALL_COUNTS + MATRIX_COUNTS + CAPPED_COUNTS

# xfer_kernel / block_copy geometry (rma.cpp apply_one / pull, copy.hip, device.hpp)
XFER_SLICE, XFER_MAX_BLOCKS = 64 << 10, 256
BYTE_SIZES = [1, 15, 17, (64 << 10) - 1, (64 << 10) + 1, 3 * (64 << 10) + 5, (16 << 20) + 19]
BYTE_DELTAS = [0, 8, 4, 2, 1]     # (dst - src) mod 16
BYTE_DST_MODS = [0, 5]            # dst mod 16
BIG_BYTE_ALIGNS = [(0, 5), (4, 0)]  # the 16 Mi size: vector branch with a head, 4-B branch

SEAM_SCRATCH = 4096   # MPIGX_RMA_SCRATCH of the chunk-seam launches
DEFAULT_SCRATCH = 4 << 20
ORDER_POSTS = 40      # envelopes per target without a flush (kRmaSlots = 16)
ORDER_COUNT = 4099
MULTI_POSTS = 20


def npdt(tname):
    return np.dtype(np.uint16) if tname == "bfloat16" else np.dtype(tname)


def esize(tname):
    return npdt(tname).itemsize


def valid(opname, tname):
    return R.valid(opname, MPI_NAME[tname])


def acc_geometry(count):
    """Blocks, threads in the grid, main-loop iterations of thread 0, number of
    threads that enter the main loop, and elements left to the tail."""
    g = max(1, min((count + ACC_U * ACC_THREADS - 1) // (ACC_U * ACC_THREADS), ACC_MAX_BLOCKS))
    nt = ACC_THREADS * g
    # thread t runs main iteration k while t + k U nt < span
    span = max(0, count - (ACC_U - 1) * nt)
    main_threads = min(nt, span)
    it0 = (span + ACC_U * nt - 1) // (ACC_U * nt)
    full, rest = divmod(span, ACC_U * nt)
    main_elems = ACC_U * (full * nt + min(rest, nt))
    return {"g": g, "nt": nt, "main_threads": main_threads, "main_iters": it0, "main_elems": main_elems,
            "tail_elems": count - main_elems, "capped": (count + 1023) // 1024 > ACC_MAX_BLOCKS}


def seam_per(scratch, n, es):
    """Elements per Get_accumulate chunk (rma.cpp win_setup slot_bytes, acc_common per)."""
    slot = max(256, (scratch // n) & ~255)
    return max(1, slot // es)


def copy_geometry(nbytes, dst_mod, src_mod):
    """Blocks of xfer_kernel and, for block 0, block_copy's branch and head."""
    want = (nbytes + XFER_SLICE - 1) // XFER_SLICE
    g = max(1, min(want, XFER_MAX_BLOCKS))
    slice_ = ((nbytes + g - 1) // g + 15) & ~15
    x = (dst_mod ^ src_mod) & 15
    if x == 0:
        branch, head = "vec16", min((16 - dst_mod) & 15, nbytes)
    elif x & 3 == 0:
        branch, head = "word4", min((4 - (dst_mod & 3)) & 3, nbytes)
    else:
        branch, head = "byte", 0
    return {"g": g, "slice": slice_, "branch": branch, "head": head, "capped": want > XFER_MAX_BLOCKS,
            "rounded": slice_ * g != nbytes and g > 1}


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
# element 0 of (window, origin) and element 1 of the origin: the op changes
# the window at element 0, and the origin shifted by one element changes it
# differently — at any count, 1 included
_HEAD_INT = {"SUM": (1, 1, 2), "PROD": (3, 2, 3), "MIN": (2, 1, 0), "MAX": (1, 2, 3), "LAND": (3, 0, 2),
             "LOR": (0, 3, 0), "LXOR": (3, 0, 2), "BAND": (3, 1, 2), "BOR": (1, 2, 4), "BXOR": (1, 2, 4),
             "REPLACE": (1, 2, 3), "NO_OP": (1, 2, 3)}
# floats: MIN / MAX start on a signed-zero pair, whose result shows which operand is the window
_HEAD_FLT = dict(_HEAD_INT, SUM=(0.5, 1.0, 2.0), PROD=(1.5, 2.0, 3.0), MIN=(0.0, -0.0, -1.0), MAX=(-0.0, 0.0, 1.0))
_PERIOD = 65537  # prime, larger than every matrix and seam count
_SPECIAL_OPS = ("MIN", "MAX", "LAND", "LOR", "LXOR", "REPLACE", "NO_OP")


def _float_specials(w, o):
    """NaN in the window only, in both, in the origin only; +0 / -0 both ways
    round; a tie — every 16 elements from element 2 on."""
    nan, k = np.float64(np.nan), w.dtype.type
    w[2::16], w[6::16] = nan, nan
    o[6::16], o[10::16] = nan, nan
    w[3::16], o[3::16] = k(-0.0), k(0.0)
    w[7::16], o[7::16] = k(0.0), k(-0.0)
    w[4::16], o[4::16] = k(2.0), k(2.0)


def operand_pair(tname, opname, count, seed):
    """Deterministic (window, origin) values of one case.  The origin has
    count + 1 elements: [:count] is the operand, [1:] the same operand shifted
    by one element (the CPU plan test uses it).  bf16 as uint16 bit patterns."""
    rng = np.random.default_rng([seed, count])
    m, g = count + 1, min(count + 1, _PERIOD)

    def ext(a):  # large counts repeat a prime period: no stride of any grid maps the pattern onto itself
        return a if g == m else np.resize(a, m)

    if tname == "bfloat16" or npdt(tname).kind == "f":
        d = np.dtype(np.float32) if tname == "bfloat16" else npdt(tname)
        w = ext((rng.integers(-4, 5, g) * 0.5).astype(d))
        o = ext((rng.integers(-4, 5, g) * 0.5).astype(d))
        if opname in _SPECIAL_OPS:
            _float_specials(w, o)
        w[0], o[0], o[1] = _HEAD_FLT[opname]
        if tname == "bfloat16":
            w, o = M.f32_to_bf16(w), M.f32_to_bf16(o)
        return w[:count].copy(), o
    d = npdt(tname)
    if d.kind == "c":
        f = np.float32 if d.itemsize == 8 else np.float64
        w = ext((rng.integers(-3, 4, g).astype(f) + 1j * rng.integers(-3, 4, g).astype(f)).astype(d))
        o = ext((rng.integers(-3, 4, g).astype(f) + 1j * rng.integers(-3, 4, g).astype(f)).astype(d))
        w[0], o[0], o[1] = {"SUM": (1 + 1j, 1, 2j), "PROD": (1 + 1j, 2, 3j)}.get(opname, (1 + 1j, 2 - 1j, 3))
        return w[:count].copy(), o
    info = np.iinfo(d)
    if opname in ("SUM", "PROD", "BAND", "BOR", "BXOR"):
        w = ext(rng.integers(info.min, info.max, g, dtype=d, endpoint=True))
        o = ext(rng.integers(info.min, info.max, g, dtype=d, endpoint=True))
        if opname in ("SUM", "PROD"):  # wraparound for certain
            w[2::16], o[2::16] = info.max, info.max
            w[3::16], o[3::16] = info.min, 3
    else:  # zeros and values other than 0 / 1
        lo = -3 if d.kind == "i" else 0
        w = ext(rng.integers(lo, 4, g).astype(d))
        o = ext(rng.integers(lo, 4, g).astype(d))
    w[0], o[0], o[1] = _HEAD_INT[opname]
    return w[:count].copy(), o


def model(tname, window, origin, opname):
    """(new window, old window) of one accumulate on one target range."""
    if tname == "bfloat16":
        old = window.copy()
        if opname == "REPLACE":
            return origin.copy(), old
        if opname == "NO_OP":
            return old.copy(), old
        return M.apply_op(opname, "BFLOAT16", window, origin), old
    return R.accumulate(window, origin, opname)


def sentinel(tname, length):
    return np.full(length * esize(tname), SENTINEL, np.uint8).view(npdt(tname)).copy()


def byte_payload(nbytes, seed):
    return np.random.default_rng([seed, nbytes]).integers(0, 256, nbytes, dtype=np.uint8)


def origin_off(tname, k):
    """Byte offset of origin view k into its allocation: 0, 4 and 20 bytes in
    turn, rounded up to the element size (a typed view starts on an element)."""
    es = esize(tname)
    return [0, (4 + es - 1) // es * es, (20 + es - 1) // es * es][k % 3]


# ---------------------------------------------------------------------------
# the plan: a list of epochs, each a list of cases on one window
# ---------------------------------------------------------------------------
def _lay(cases):
    """Assign every case its range: GUARD | range | GUARD | range | ... | GUARD,
    every range starting on a multiple of 16 elements; returns the length."""
    at = GUARD
    for c in cases:
        c["at"] = at
        at = (at + c["count"] + GUARD + 15) // 16 * 16
    return at


def _epoch(section, tname, sync, cases, shape="disjoint"):
    return {"section": section, "type": tname, "sync": sync, "shape": shape, "cases": cases,
            "length": _lay(cases) if shape == "disjoint" else None}


def _acc(kind, tname, op, count, k):
    return {"kind": kind, "type": tname, "op": op, "count": count, "ooff": origin_off(tname, k)}


def _minmax_or(tname, other):
    return "MAX" if valid("MAX", tname) else other


def plan_matrix(counts=tuple(MATRIX_COUNTS), capped=True):
    """a. every valid (op, type) as Accumulate and Get_accumulate at the
    loop-reaching counts; one type of each element size at 1, 255 and the two
    capped counts (Accumulate, whose launch is not cut into chunks; an
    arithmetic and a MIN / MAX op — complex128 has no MIN / MAX and takes
    REPLACE; Get_accumulate SUM at the larger one crosses the default slot)."""
    eps, k = [], 0
    for t in TYPES:
        for op in OPS:
            if not valid(op, t):
                continue
            cases = []
            for kind in ("acc", "gacc"):
                for cnt in counts:
                    cases.append(_acc(kind, t, op, cnt, k))
                    k += 1
            eps.append(_epoch("a", t, "fence", cases))
    if capped:
        for t in SIZE_TYPES:
            ops = ("SUM", _minmax_or(t, "REPLACE"))
            eps.append(_epoch("a", t, "fence", [_acc(kind, t, op, cnt, i) for i, (kind, op, cnt) in enumerate(
                (kd, op, cnt) for kd in ("acc", "gacc") for op in ops for cnt in SMALL_COUNTS)]))
            for cnt in CAPPED_COUNTS:
                for op in ops:
                    eps.append(_epoch("a", t, "fence", [_acc("acc", t, op, cnt, k)]))
                    k += 1
            eps.append(_epoch("a", t, "lock", [_acc("gacc", t, "SUM", CAPPED_COUNTS[1], 1)]))
    return eps


def plan_seams(n, scratch=SEAM_SCRATCH):
    """b. Get_accumulate at per - 1, per, per + 1 and 3 per + 7 elements."""
    eps = []
    for t in SIZE_TYPES:
        per = seam_per(scratch, n, esize(t))
        for op in ("SUM", "REPLACE", "NO_OP"):
            eps.append(_epoch("b", t, "lock", [dict(_acc("gacc", t, op, cnt, i), per=per) for i, cnt in
                                               enumerate((per - 1, per, per + 1, 3 * per + 7))]))
    for t in ("bfloat16", "complex128"):
        eps.append(_epoch("b", t, "lock", [_acc("fop", t, "SUM", 1, 0)]))
    return eps


def byte_aligns(nbytes, sweep="full"):
    if nbytes == BYTE_SIZES[-1]:
        return BIG_BYTE_ALIGNS
    if sweep == "one":  # one alignment of every branch, with and without a head
        return [(0, 5), (4, 5), (1, 0)] if nbytes == BYTE_SIZES[5] else []
    return [(d, m) for d in BYTE_DELTAS for m in BYTE_DST_MODS]


def plan_bytes(sweep="full"):
    """c. Put and Get on a uint8 window, under a fence epoch and lock / unlock."""
    eps = []
    for nbytes in BYTE_SIZES:
        if sweep == "one" and nbytes != BYTE_SIZES[5]:
            continue
        for kind in ("put", "get"):
            for sync in ("fence", "lock"):
                cases = [{"kind": kind, "type": "uint8", "op": None, "count": nbytes + 16, "nbytes": nbytes,
                          "delta": d, "dst_mod": m, "src_mod": (m - d) % 16} for d, m in byte_aligns(nbytes, sweep)]
                eps.append(_epoch("c", "uint8", sync, cases))
    return eps


ORDER_OPS = {"float32": ["REPLACE", "SUM", "PROD", "MAX", "MIN"], "int64": ["BXOR", "SUM"]}
MULTI_OPS = ["SUM", "BOR", "MAX"]


def order_starts():
    """Start of each of the ORDER_POSTS overlapping ranges inside the payload."""
    return [(j * 331) % 1025 for j in range(ORDER_POSTS)]


def plan_order():
    """d. ORDER_POSTS accumulates per target without a flush, on overlapping
    ranges, ops that do not commute; then every rank into the same ranges of
    rank 0 with order-independent integer ops."""
    eps = []
    for t in ("float32", "int64"):
        for sync in ("fence", "lock"):
            eps.append({"section": "d", "type": t, "sync": sync, "shape": "order",
                        "length": GUARD + 1025 + ORDER_COUNT + GUARD,
                        "cases": [{"kind": "order", "type": t, "op": "+".join(ORDER_OPS[t]), "count": ORDER_COUNT}]})
    eps.append({"section": "d", "type": "int64", "sync": "fence", "shape": "multi",
                "length": GUARD + len(MULTI_OPS) * (ORDER_COUNT + GUARD),
                "cases": [{"kind": "multi", "type": "int64", "op": "+".join(MULTI_OPS), "count": ORDER_COUNT}]})
    return eps


def order_operand(t, j, seed):
    """Origin of post j of the order epoch: f32 half-integers (PROD by +-1 /
    +-2 so magnitudes stay small), full-range int64."""
    rng = np.random.default_rng([seed, j, 77])
    op = ORDER_OPS[t][j % len(ORDER_OPS[t])]
    if t == "float32":
        if op == "PROD":
            return op, rng.choice(np.array([1, -1, 2, -2], np.float32), ORDER_COUNT)
        return op, (rng.integers(-4, 5, ORDER_COUNT) * 0.5).astype(np.float32)
    return op, rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, ORDER_COUNT, dtype=np.int64, endpoint=True)


def multi_operand(j, who):
    rng = np.random.default_rng([who, j, 78])
    op = MULTI_OPS[j % len(MULTI_OPS)]
    return op, rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, ORDER_COUNT, dtype=np.int64, endpoint=True)


def plan(n, sections, scratch=DEFAULT_SCRATCH):
    """Epochs of the named sections: 'a' matrix, 'a4099' its 4099-count row,
    'b' seams, 'c' byte paths, 'c1' one alignment sweep, 'd' order."""
    eps = []
    for s in sections:
        if s == "a":
            eps += plan_matrix()
        elif s == "a4099":
            eps += plan_matrix(counts=(4099,), capped=False)
        elif s == "b":
            eps += plan_seams(n, scratch)
        elif s == "c":
            eps += plan_bytes()
        elif s == "c1":
            eps += plan_bytes("one")
        elif s == "d":
            eps += plan_order()
        else:
            raise ValueError(s)
    for i, ep in enumerate(eps):
        ep["id"] = i
        for j, c in enumerate(ep["cases"]):
            c["id"] = f"{ep['section']}{i}.{j} {c['kind']} {c['type']} {c['op']} x{c['count']}"
            c["seed"] = 1000 * i + j
    return eps


def ncases(eps):
    return sum(len(ep["cases"]) for ep in eps)


def window_elems(eps, tname):
    return max(ep["length"] for ep in eps if ep["type"] == tname)
