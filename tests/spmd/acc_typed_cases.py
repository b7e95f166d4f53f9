"""Case table and model of Accumulate / Get_accumulate through non-contiguous
derived datatypes, shared by the CPU tests (tests/test_acc_typed_cpu.py), the
worker (tests/spmd/acc_typed_worker.py, on numpy windows under MPICH for the
fixture and on device windows for the GPU test) and the GPU test.

Every side of a case (origin, target, result) is a type DESCRIPTION plus an
instance count; `elem_offsets` turns a description into the element offsets of
its type map by the MPI rules (vector, hvector, subarray, resized, struct) —
nobody asks the engine.  The model gathers the target's elements through the
target map, applies oracle/rma_model.accumulate with the origin's elements
gathered through the origin map, scatters the new values back and scatters
the old ones through the result map.  Windows, origin and result buffers
start as the SENTINEL byte everywhere, so every byte outside a type map must
come back as it was; every comparison is over whole allocations.

Rank r targets (r + 1) % n (one origin per window) except the `multi` case,
where every rank accumulates into rank 0.  Counts come from the launch
arithmetic of acc_typed_kernel (common.hpp kAccTypedU / kAccTypedGridCap,
rma.cpp apply_one: g = clamp(ceil(count / 1024), 1, 1024) blocks of 256
threads, a 4-way unrolled grid-stride main loop and a tail: `geometry`) and
from the Get_accumulate chunking (per = slot_bytes / esize elements per
envelope, chunk k posted with first = k * per: `seams`).
"""
import hashlib

import numpy as np

import rma_data_cases as D
from oracle import rma_model as R

N = 3                 # ranks of the fixture and of the GPU test
SCRATCH = 4096        # MPIGX_RMA_SCRATCH: 1280-byte slots at n = 3
SENTINEL = D.SENTINEL
GUARD = 16            # sentinel elements before the target displacement and after the span
RUN_CAP = 64          # kRmaRunCap: runs of a non-contiguous target type

# acc_typed_kernel launch geometry (common.hpp, rma.cpp apply_one)
THREADS, U, GRID_CAP = 256, 4, 1024

MPI_ERR_TYPE, MPI_ERR_RMA_RANGE = 3, 55

npdt, esize = D.npdt, D.esize
MPI_TYPE = dict(D.MPI_NAME)  # type name -> MPI datatype name


# ---------------------------------------------------------------------------
# type descriptions
# ---------------------------------------------------------------------------
def contig():
    return {"k": "contig"}


def vector(count, bl, stride):
    return {"k": "vector", "count": count, "bl": bl, "stride": stride}


def hvector(count, bl, stride_bytes):
    return {"k": "hvector", "count": count, "bl": bl, "stride_bytes": stride_bytes}


def subarray(sizes, sub, start):
    """Row-major (MPI_ORDER_C) 2-D subarray."""
    return {"k": "subarray", "sizes": list(sizes), "sub": list(sub), "start": list(start)}


def resized(base, extent_el):
    """lb 0, extent `extent_el` ELEMENTS."""
    return {"k": "resized", "base": base, "extent_el": extent_el}


def struct(bl, disp_el):
    """Blocks of one type: lengths and displacements in ELEMENTS (first at 0)."""
    return {"k": "struct", "bl": list(bl), "disp_el": list(disp_el)}


def elem_offsets(desc, es):
    """(byte offsets of one instance's elements in type-map order, extent in bytes)."""
    k = desc["k"]
    if k == "contig":
        return np.array([0], np.int64), es
    if k in ("vector", "hvector"):
        st = desc["stride"] * es if k == "vector" else desc["stride_bytes"]
        off = (np.arange(desc["count"], dtype=np.int64)[:, None] * st +
               np.arange(desc["bl"], dtype=np.int64)[None, :] * es).reshape(-1)
        return off, (desc["count"] - 1) * st + desc["bl"] * es
    if k == "subarray":
        (_, cols), (sr, sc), (r0, c0) = desc["sizes"], desc["sub"], desc["start"]
        off = ((r0 + np.arange(sr, dtype=np.int64))[:, None] * cols + c0 + np.arange(sc, dtype=np.int64)[None, :])
        return off.reshape(-1) * es, desc["sizes"][0] * cols * es
    if k == "resized":
        return elem_offsets(desc["base"], es)[0], desc["extent_el"] * es
    if k == "struct":
        assert desc["disp_el"][0] == 0
        off = np.concatenate([d + np.arange(b, dtype=np.int64) for b, d in zip(desc["bl"], desc["disp_el"])])
        return off * es, max(d + b for b, d in zip(desc["bl"], desc["disp_el"])) * es
    raise ValueError(k)


def stream_offsets(side, es):
    """ELEMENT offsets of the packed stream of `count` instances of a side."""
    desc, count = side
    off, ext = elem_offsets(desc, es)
    assert ext % es == 0 and not (off % es).any()
    return ((np.arange(count, dtype=np.int64)[:, None] * ext + off[None, :]) // es).reshape(-1)


def span_elems(side, es):
    o = stream_offsets(side, es)
    return int(o.max()) + 1 if o.size else 0


def instance_elems(side, es):
    return elem_offsets(side[0], es)[0].size


def run_starts(side, es):
    """Stream indices at which a new contiguous block of the map starts."""
    o = stream_offsets(side, es)
    return set((np.flatnonzero(np.diff(o) != 1) + 1).tolist()) | {0}


def nruns(desc):
    """Runs the engine flattens one instance to (types.cpp append): one per
    progression of equal blocks; the descriptions here use unequal blocks
    where more than one run is wanted."""
    if desc["k"] == "struct":
        return len(desc["bl"])
    return nruns(desc["base"]) if desc["k"] == "resized" else 1


def build(MPI, desc, tname):
    """The description as a committed MPI datatype of the mirror."""
    base = getattr(MPI, MPI_TYPE[tname])
    T, es, k = MPI.Types, esize(tname), desc["k"]
    if k == "contig":
        return base
    if k == "vector":
        t = T.create_vector(desc["count"], desc["bl"], desc["stride"], base)
    elif k == "hvector":
        t = T.create_hvector(desc["count"], desc["bl"], desc["stride_bytes"], base)
    elif k == "subarray":
        t = T.create_subarray(desc["sizes"], desc["sub"], desc["start"], base, rowmajor=True)
    elif k == "resized":
        t = T.create_resized(build(MPI, desc["base"], tname), 0, desc["extent_el"] * es)
    elif k == "struct":
        t = T.create_struct(desc["bl"], [d * es for d in desc["disp_el"]], [base] * len(desc["bl"]))
    else:
        raise ValueError(k)
    return T.commit_(t)


# ---------------------------------------------------------------------------
# launch geometry and chunk seams
# ---------------------------------------------------------------------------
def geometry(count):
    """As rma_data_cases.acc_geometry, with acc_typed_kernel's constants."""
    g = max(1, min((count + U * THREADS - 1) // (U * THREADS), GRID_CAP))
    nt = THREADS * g
    span = max(0, count - (U - 1) * nt)
    full, rest = divmod(span, U * nt)
    main_elems = U * (full * nt + min(rest, nt))
    return {"g": g, "nt": nt, "main_elems": main_elems, "tail_elems": count - main_elems,
            "capped": (count + U * THREADS - 1) // (U * THREADS) > GRID_CAP}


def per_of(tname, n=N, scratch=SCRATCH):
    return D.seam_per(scratch, n, esize(tname))


def seams(count, per):
    """Stream indices where a new Get_accumulate chunk starts (first = k * per)."""
    return list(range(per, count, per))


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def _case(name, tname, op, kind, o, t, r=None, **kw):
    c = {"id": name, "type": tname, "op": op, "kind": kind, "o": o, "t": t, "r": r, "disp": GUARD, "dyn": False,
         "mpich": tname != "bfloat16", "shape": "one"}
    es = esize(tname)
    c["count"] = stream_offsets(t, es).size
    c["wlen"] = c["disp"] + span_elems(t, es) + GUARD
    c.update(kw)
    return c


def _seam_cases():
    out = []
    p4, p8 = per_of("float32"), per_of("int64")
    assert (p4, p8) == (320, 160), (p4, p8)
    # 4-byte type: one instance each; 321 and 967 cut blocks of 3 / 400 / 300 / 267 elements
    t4 = {p4 - 1: (vector(29, 11, 13), 1), p4: (vector(32, 10, 12), 1), p4 + 1: (vector(107, 3, 5), 1),
          3 * p4 + 7: (struct([400, 300, 267], [0, 410, 720]), 1)}
    for cnt, t in t4.items():
        out.append(_case(f"seam4 x{cnt}", "float32", "REPLACE", "gacc", (contig(), cnt), t, (contig(), cnt), per=p4))
    # 8-byte type: many instances; 161 cuts instance 22 of 23 inside its second block
    t8 = {p8 - 1: (struct([2, 1], [0, 3]), 53), p8: (vector(4, 2, 3), 20), p8 + 1: (struct([4, 3], [0, 5]), 23),
          3 * p8 + 7: (struct([200, 287], [0, 210]), 1)}
    for cnt, t in t8.items():
        out.append(_case(f"seam8 x{cnt}", "int64", "BXOR", "gacc", (contig(), cnt), t, (vector(cnt, 1, 2), 1), per=p8))
    return out


def _cases():
    cs = []
    big = ((1 << 20) + 517 + 2) // 3  # blocks of 3 int8: past the grid cap, about 1.4 MB of window
    run64 = struct([1 + i % 3 for i in range(64)], np.cumsum([0] + [2 + i % 3 for i in range(63)]).tolist())
    cs += [
        # layouts
        _case("contig->vector", "float32", "SUM", "acc", (contig(), 100), (vector(50, 2, 3), 1)),
        _case("subarray->subarray, result vector", "float64", "SUM", "gacc", (subarray([8, 10], [4, 6], [2, 3]), 1),
              (subarray([6, 12], [3, 8], [1, 2]), 1), (vector(12, 2, 5), 1)),
        _case("resized vector x3 interleaved", "int32", "MAX", "acc", (contig(), 12),
              (resized(vector(4, 1, 3), 1), 3)),
        _case("struct 4 unequal runs x2", "int64", "BXOR", "gacc", (contig(), 22),
              (struct([3, 1, 5, 2], [0, 5, 8, 16]), 2), (contig(), 22)),
        _case("struct 64 runs", "int16", "SUM", "acc", (vector(127, 1, 2), 1), (run64, 1)),
        _case("dynamic window hvector", "float32", "REPLACE", "acc", (contig(), 30), (hvector(10, 3, 20), 1),
              dyn=True),
        _case("complex128 vector, result hvector", "complex128", "SUM", "gacc", (contig(), 10),
              (vector(5, 2, 3), 1), (hvector(10, 1, 48), 1)),
        _case("NO_OP typed fetch", "int32", "NO_OP", "gacc", (contig(), 24), (subarray([5, 9], [4, 6], [1, 2]), 1),
              (vector(8, 3, 4), 1)),
        # bf16: against the model only (MPICH has no handle for it)
        _case("bf16 contig->vector", "bfloat16", "SUM", "acc", (contig(), 60), (vector(20, 3, 5), 1)),
        _case("bf16 vector->struct, result vector", "bfloat16", "REPLACE", "gacc", (vector(11, 2, 3), 1),
              (struct([3, 1, 5, 2], [0, 5, 8, 16]), 2), (vector(22, 1, 2), 1)),
        # loop regions of acc_typed_kernel
        _case("1 element", "float32", "SUM", "acc", (contig(), 1), (resized(contig(), 2), 1)),
        _case("tail only x700", "int32", "SUM", "acc", (contig(), 700), (vector(700, 1, 2), 1)),
        _case("body and tail x1000", "float64", "SUM", "acc", (vector(1000, 1, 2), 1), (vector(500, 2, 3), 1)),
        _case("past the grid cap", "int8", "SUM", "acc", (contig(), 3 * big), (vector(big, 3, 4), 1)),
    ]
    cs += _seam_cases()
    # ordering
    cs.append(_case("REPLACE then SUM, overlapping, no flush", "float32", "REPLACE+SUM", "acc", (contig(), 40),
                    (vector(20, 2, 4), 1), shape="order", wlen=GUARD + 1 + 78 + GUARD))
    cs.append(_case("SUM from every rank into rank 0", "int64", "SUM", "acc", (contig(), 48), (vector(16, 3, 5), 1),
                    shape="multi"))
    for i, c in enumerate(cs):
        c["seed"] = 7000 + i
    return cs


CASES = _cases()
ORDER_SHIFT = 1  # the SUM of the order case lands one element after the REPLACE

# Refusals (engine only): expected class, window untouched.  `o` / `t` as in
# a case; `otype` / `ttype` name the element type of each side; `mixed`: the
# target is a struct of an int32 block and a float32 block with a hole.
REFUSALS = [
    {"id": "mixed-basic struct", "otype": "int32", "ttype": "int32", "o": (contig(), 4), "t": None, "mixed": True,
     "want": MPI_ERR_TYPE},
    {"id": "basic-type mismatch", "otype": "int32", "ttype": "float32", "o": (contig(), 12), "t": (vector(6, 2, 3), 1),
     "want": MPI_ERR_TYPE},
    {"id": "element-count mismatch", "otype": "float32", "ttype": "float32", "o": (contig(), 10),
     "t": (vector(6, 2, 3), 1), "want": MPI_ERR_TYPE},
    {"id": "65-run target", "otype": "int16", "ttype": "int16", "o": (contig(), 129),
     "t": (struct([1 + i % 3 for i in range(65)], np.cumsum([0] + [2 + i % 3 for i in range(64)]).tolist()), 1),
     "want": MPI_ERR_TYPE},
    {"id": "hvector of FLOAT, 6-byte stride", "otype": "float32", "ttype": "float32", "o": (contig(), 3),
     "t": (hvector(3, 1, 6), 1), "want": MPI_ERR_TYPE},
    {"id": "span leaves the window", "otype": "float32", "ttype": "float32", "o": (contig(), 12),
     "t": (vector(6, 2, 3), 1), "want": MPI_ERR_RMA_RANGE, "past": True},
]


def window_elems(tname):
    return max(c["wlen"] for c in CASES if c["type"] == tname and not c["dyn"])


# ---------------------------------------------------------------------------
# inputs and model
# ---------------------------------------------------------------------------
def sentinel(tname, length):
    return D.sentinel(tname, length)


def _op_of(c, j=0):
    return c["op"].split("+")[j]


def operands(c, who, j=0):
    """(window values, origin values) of the `count` elements of post j issued
    by rank `who` (the window values are those of `who`'s TARGET before post 0).
    The order case draws plain values for both posts: a NaN stored by the
    REPLACE would make the SUM's result depend on NaN-payload rules."""
    gen = "SUM" if c["shape"] == "order" else _op_of(c, j)
    w, o = D.operand_pair(c["type"], gen, c["count"], c["seed"] * 64 + who * 4 + j)
    return w, o[:c["count"]]


def origin_buffer(c, who, j=0):
    """Whole origin allocation of rank `who`: sentinel, the operand through the origin map."""
    es = esize(c["type"])
    buf = sentinel(c["type"], span_elems(c["o"], es) + 2)
    buf[stream_offsets(c["o"], es)] = operands(c, who, j)[1]
    return buf


def result_buffer(c):
    return sentinel(c["type"], span_elems(c["r"], esize(c["type"])) + 2) if c["r"] else None


def window_init(c, me, n, length=None):
    """Whole window of rank `me` before the case: sentinel, the case's window
    operand (drawn with its ORIGIN's seed) through the target map at disp."""
    es = esize(c["type"])
    win = sentinel(c["type"], length or c["wlen"])
    src = me if c["shape"] == "multi" else (me - 1) % n
    if c["shape"] == "multi" and me != 0:
        return win
    idx = c["disp"] + stream_offsets(c["t"], es)
    if c["shape"] == "order":  # the union of the two posts' maps
        idx = np.union1d(idx, idx + ORDER_SHIFT)
        win[idx] = D.operand_pair(c["type"], "SUM", idx.size, c["seed"] * 64 + src * 4 + 3)[0]
        return win
    win[idx] = operands(c, src)[0]
    return win


def _apply(c, win, idx, origin, op):
    if c["type"] == "bfloat16":
        new, old = D.model("bfloat16", win[idx], origin, op)
    else:
        new, old = R.accumulate(win[idx], origin, op)
    win[idx] = new
    return old


def model(c, me, n, length=None, offsets=None):
    """(whole window of rank `me` after the case, whole result buffer of rank
    `me` as origin or None).  `offsets`: element offsets to use for the target
    instead of its type map (the CPU test's contiguous counter-model)."""
    es = esize(c["type"])
    win = window_init(c, me, n, length)
    toff = stream_offsets(c["t"], es) if offsets is None else offsets
    if c["shape"] == "multi":
        if me == 0:
            for who in range(n):
                _apply(c, win, c["disp"] + toff, operands(c, who)[1], "SUM")
        return win, None
    src, tgt = (me - 1) % n, (me + 1) % n
    if c["shape"] == "order":
        for j in range(2):
            _apply(c, win, c["disp"] + j * ORDER_SHIFT + toff, operands(c, src, j)[1], _op_of(c, j))
        return win, None
    _apply(c, win, c["disp"] + toff, operands(c, src)[1], c["op"])
    res = None
    if c["kind"] == "gacc":
        # what I fetch: my target's window values before my accumulate
        res = result_buffer(c)
        res[stream_offsets(c["r"], es)] = window_init(c, tgt, n, length)[c["disp"] + stream_offsets(c["t"], es)]
    return win, res


def enc(a):
    """Exact record of a whole allocation: its bytes as hex, or their SHA-256
    when that would be long (the fixture stays small; equality is still bit
    for bit)."""
    b = np.ascontiguousarray(a).view(np.uint8).tobytes()
    return b.hex() if len(b) <= 256 else "sha256:" + hashlib.sha256(b).hexdigest()
