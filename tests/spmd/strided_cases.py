"""Derived datatypes in the v-collectives and in one-sided Get / Put: the
scenarios as data, and a numpy restatement of MPI's type map that says what
every buffer must hold afterwards.

`ops(n)` lists the operations of an n-rank run; each one carries every rank's
arguments, so tests/spmd/strided_worker.py executes its own rank's share (on
numpy arrays under MPICH for the fixture, on device tensors under libmpigx)
and `expected(n)` plays all ranks at once with `pack` / `unpack` below.  The
fixture (tests/golden/strided_golden.json) must equal `expected` record for
record (tests/test_strided_cpu.py), which pins both independently of the
engine.

A type is a spec: a numpy dtype (predefined, or a struct by its fields), or
("vector", count, blocklength, stride, old), ("contig", count, old),
("subarray", sizes, subsizes, starts, old) in C order, ("resized", old, lb,
extent).  Receive buffers and windows start as 0xEE."""
import numpy as np

BOUNDARY = np.dtype([("c", np.uint16), ("a", np.int64), ("b", np.uint8)], align=True)  # size 11, extent 24
NTUPLE3 = np.dtype([("f0", np.uint8), ("f1", np.uint8), ("f2", np.uint8)])
FILL = 0xEE
TAB = [2, 0, 3, 1]  # ragged counts with a zero


# ---------------------------------------------------------------------------
# type maps
# ---------------------------------------------------------------------------
def typemap(spec):
    """(byte offsets in pack order, lb, extent) of one instance."""
    if isinstance(spec, np.dtype):
        if spec.fields is None:
            return np.arange(spec.itemsize, dtype=np.int64), 0, spec.itemsize
        offs = [spec.fields[nm][1] + typemap(spec.fields[nm][0])[0] for nm in spec.names]
        return np.concatenate(offs), 0, spec.itemsize
    kind = spec[0]
    if kind == "vector":
        _, count, bl, stride, old = spec
        o, lb, ext = typemap(old)
        offs = [(i * stride + j) * ext + o for i in range(count) for j in range(bl)]
        return np.concatenate(offs), lb, ((count - 1) * stride + bl) * ext
    if kind == "contig":
        _, count, old = spec
        o, lb, ext = typemap(old)
        return np.concatenate([j * ext + o for j in range(count)]), lb, count * ext
    if kind == "subarray":
        _, sizes, subsizes, starts, old = spec
        o, _, ext = typemap(old)
        idx = np.indices(subsizes).reshape(len(sizes), -1)
        lin = np.zeros(idx.shape[1], dtype=np.int64)
        for d in range(len(sizes)):
            lin = lin * sizes[d] + idx[d] + starts[d]
        return (lin[:, None] * ext + o[None, :]).reshape(-1), 0, int(np.prod(sizes)) * ext
    if kind == "resized":
        _, old, lb, extent = spec
        return typemap(old)[0], lb, extent
    raise ValueError(spec)


def size_of(spec):
    return len(typemap(spec)[0])


def span(spec, count):
    """True bounds [lo, hi) of `count` instances, in bytes from the pointer."""
    o, _, ext = typemap(spec)
    return int(o.min()), int(o.max()) + 1 + (count - 1) * ext


def addrs(spec, count, disp=0):
    o, _, ext = typemap(spec)
    return ((disp + np.arange(count, dtype=np.int64))[:, None] * ext + o[None, :]).reshape(-1)


def pack(buf, spec, count, disp=0):
    return buf[addrs(spec, count, disp)].copy()


def unpack(buf, data, spec, count, disp=0):
    a = addrs(spec, count, disp)
    assert len(a) == len(data), (len(a), len(data))
    buf[a] = data


def build(MPI, spec):
    """The committed MPI.Datatype of a spec."""
    T = MPI.Types
    if isinstance(spec, np.dtype):
        return MPI.Datatype(spec)
    kind = spec[0]
    if kind == "vector":
        return T.commit_(T.create_vector(spec[1], spec[2], spec[3], build(MPI, spec[4])))
    if kind == "contig":
        return T.commit_(T.create_contiguous(spec[1], build(MPI, spec[2])))
    if kind == "subarray":
        return T.commit_(T.create_subarray(list(spec[1]), list(spec[2]), list(spec[3]), build(MPI, spec[4]),
                                           rowmajor=True))
    if kind == "resized":
        return T.commit_(T.create_resized(build(MPI, spec[1]), spec[2], spec[3]))
    raise ValueError(spec)


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------
def data(nbytes, seed):
    return ((np.arange(nbytes, dtype=np.int64) * 7 + 3 + 37 * seed) % 251).astype(np.uint8)


def blank(nbytes):
    return np.full(nbytes, FILL, np.uint8)


def prefix(counts):
    return [int(x) for x in np.cumsum([0] + list(counts))[:-1]]


def side(buf, spec, off=0):
    """One rank's side of a collective: the bytes of its buffer, the datatype
    and the byte offset of the pointer it passes into that buffer."""
    return {"buf": buf, "spec": spec, "off": off}


def room(spec, count, off=0):
    return off + (span(spec, count)[1] if count else 0) + 8


def coll(kind, name, n, sspec, rspec, counts, root=0, inplace=False, soff=0, roff=0):
    """A v-collective in which every rank uses the same pair of types.  counts:
    per-rank list (gatherv / scatterv / allgatherv) or matrix [r][q] = what r
    sends to q (alltoallv)."""
    ranks = []
    for r in range(n):
        if kind == "gatherv":
            s = side(data(room(sspec, counts[r], soff), r), sspec, soff)
            v = side(blank(room(rspec, sum(counts), roff)), rspec, roff) if r == root else None
            if inplace and r == root:
                unpack(v["buf"][roff:], pack(s["buf"][soff:], sspec, counts[r]), rspec, counts[r], prefix(counts)[r])
                s = None
        elif kind == "scatterv":
            s = side(data(room(sspec, sum(counts), soff), 40 + r), sspec, soff) if r == root else None
            v = side(blank(room(rspec, counts[r], roff)), rspec, roff)
        elif kind == "allgatherv":
            s = side(data(room(sspec, counts[r], soff), 80 + r), sspec, soff)
            v = side(blank(room(rspec, sum(counts), roff)), rspec, roff)
            if inplace:
                unpack(v["buf"][roff:], pack(s["buf"][soff:], sspec, counts[r]), rspec, counts[r], prefix(counts)[r])
                s = None
        else:
            s = side(data(room(sspec, sum(counts[r]), soff), 120 + r), sspec, soff)
            v = side(blank(room(rspec, sum(counts[q][r] for q in range(n)), roff)), rspec, roff)
        ranks.append({"send": s, "recv": v})
    return {"kind": kind, "name": name, "root": root, "counts": counts, "ranks": ranks}


def split(total, n):
    """Uneven shares of `total` columns."""
    return [total // n + (1 if r < total % n else 0) for r in range(n)]


def ops(n):
    out = []
    ragged = [TAB[r % 4] for r in range(n)]
    a2a = [[TAB[(r + q) % 4] for q in range(n)] for r in range(n)]
    # struct arrays, as MPI.jl's Gatherv! / Scatterv! / Allgatherv! / Alltoallv! pass Datatype(eltype(buf))
    for nm, T in (("boundary", BOUNDARY), ("ntuple3", NTUPLE3)):
        out.append(coll("gatherv", f"gatherv_{nm}", n, T, T, ragged, root=n - 1))
        out.append(coll("scatterv", f"scatterv_{nm}", n, T, T, ragged, root=0))
        out.append(coll("allgatherv", f"allgatherv_{nm}", n, T, T, ragged))
        out.append(coll("alltoallv", f"alltoallv_{nm}", n, T, T, a2a))
    out.append(coll("gatherv", "gatherv_boundary_inplace", n, BOUNDARY, BOUNDARY, ragged, root=0, inplace=True))
    # columns of a row-major R x C matrix: one resized-vector instance per column at the root, contiguous leaves
    R, C = 5, 7
    cols = split(C, n)
    for nm, el, off in (("f64", np.dtype("f8"), 0), ("i16", np.dtype("i2"), 0), ("c128", np.dtype("c16"), 0),
                        ("c128_off8", np.dtype("c16"), 8)):
        col = ("resized", ("vector", R, 1, C, el), 0, el.itemsize)
        leaf = ("contig", R, el)
        out.append(coll("scatterv", f"columns_scatterv_{nm}", n, col, leaf, cols, root=0, soff=off))
        out.append(coll("gatherv", f"columns_gatherv_{nm}", n, leaf, col, cols, root=0, roff=off))
    # Alltoallv: vector <-> contiguous
    f4 = np.dtype("f4")
    vec, two = ("vector", 2, 1, 3, f4), ("contig", 2, f4)
    out.append(coll("alltoallv", "alltoallv_vector_to_contig", n, vec, two, a2a))
    out.append(coll("alltoallv", "alltoallv_contig_to_vector", n, two, vec, a2a))
    # Allgatherv into a 2-D subarray type, and IN_PLACE with a vector type
    i4 = np.dtype("i4")
    sub = ("subarray", (4, 6), (2, 3), (1, 2), i4)
    out.append(coll("allgatherv", "allgatherv_subarray", n, ("contig", 6, i4), sub, ragged))
    out.append(coll("allgatherv", "allgatherv_inplace_vector", n, vec, vec, ragged, inplace=True))
    out.append(rma_ops(n))
    return out


def xfer(what, origin, target, disp, obuf, ospec, ocount, tspec, tcount, dyn=False):
    return {"what": what, "origin": origin, "target": target, "disp": disp, "obuf": obuf, "ospec": ospec,
            "ocount": ocount, "tspec": tspec, "tcount": tcount, "dyn": dyn}


WIN_BYTES = 1024


def rma_ops(n):
    """One window of WIN_BYTES per rank (disp_unit 1) plus one dynamic window
    with one attached region per rank; epoch 1 = Puts, epoch 2 = Gets.  Every
    rank r is the origin of the same list towards t = (r + 1) % n."""
    i4, f8 = np.dtype("i4"), np.dtype("f8")
    vec = ("vector", 3, 2, 4, i4)                    # 24 B out of 40
    face = ("subarray", (4, 6), (4, 1), (0, 5), f8)  # the last column of a 4 x 6 tile: a halo face
    cube = ("subarray", (3, 4, 5), (2, 2, 3), (1, 0, 2), np.dtype("i2"))
    puts, gets = [], []
    for r in range(n):
        t = (r + 1) % n
        k = 10 * r
        puts += [
            xfer("put", r, t, 0, data(64, k + 1), vec, 1, ("contig", 6, i4), 1),       # vector -> contiguous
            xfer("put", r, t, 64, data(32, k + 2), ("contig", 4, f8), 1, face, 1),     # contiguous -> halo face
            xfer("put", r, t, 288, data(96, k + 3), BOUNDARY, 3, BOUNDARY, 3),         # struct -> struct
            xfer("put", r, t, 400, data(16, k + 9), NTUPLE3, 4, NTUPLE3, 4),
            xfer("put", r, t, 448, data(32, k + 4), i4, 8, ("vector", 4, 1, 2, i4), 2),  # 8 x 4 B = 2 x 16 B
            xfer("put", r, -1, 0, data(64, k + 5), vec, 1, vec, 1),                    # PROC_NULL
            # two Puts of one origin to overlapping target bytes in one epoch: the later one wins
            xfer("put", r, t, 520, data(64, k + 6), vec, 1, vec, 1),
            xfer("put", r, t, 524, data(64, k + 7), vec, 1, vec, 1),
            xfer("put", r, t, 32, data(64, k + 8), vec, 1, ("vector", 3, 1, 3, f8), 1, dyn=True),  # absolute address
        ]
        gets += [
            xfer("get", r, t, 600, blank(24), ("contig", 12, np.dtype("i2")), 1, cube, 1),  # 3-D subarray -> contiguous
            xfer("get", r, t, 288, blank(96), BOUNDARY, 3, BOUNDARY, 3),
            xfer("get", r, t, 400, blank(16), NTUPLE3, 4, NTUPLE3, 4),
            xfer("get", r, t, 0, blank(64), vec, 1, ("contig", 6, i4), 1),
            xfer("get", r, -1, 0, blank(24), ("contig", 6, i4), 1, ("contig", 6, i4), 1),
            xfer("get", r, t, 32, blank(64), vec, 1, ("vector", 3, 1, 3, f8), 1, dyn=True),
        ]
    win = [blank(WIN_BYTES) for _ in range(n)]
    for r in range(n):
        win[r][600:600 + 120] = data(120, 200 + r)  # what the cube Get reads
    return {"kind": "rma", "name": "rma", "win": win, "dyn": [blank(128) for _ in range(n)], "puts": puts,
            "gets": gets}


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def hexof(a):
    return None if a is None else np.ascontiguousarray(a).tobytes().hex()


def expected(n):
    """[rank][op] -> record, as strided_worker.py writes them."""
    recs = [[] for _ in range(n)]
    for op in ops(n):
        kind, ranks, counts = op["kind"], op.get("ranks"), op.get("counts")
        if kind == "rma":
            win = [w.copy() for w in op["win"]]
            dyn = [d.copy() for d in op["dyn"]]
            got = [[] for _ in range(n)]
            for x in op["puts"]:
                if x["target"] < 0:
                    continue
                dst = (dyn if x["dyn"] else win)[x["target"]]
                unpack(dst[x["disp"]:], pack(x["obuf"], x["ospec"], x["ocount"]), x["tspec"], x["tcount"])
            for x in op["gets"]:
                o = x["obuf"].copy()
                if x["target"] >= 0:
                    src = (dyn if x["dyn"] else win)[x["target"]]
                    unpack(o, pack(src[x["disp"]:], x["tspec"], x["tcount"]), x["ospec"], x["ocount"])
                got[x["origin"]].append(hexof(o))
            for r in range(n):
                recs[r].append({"case": op["name"], "win": hexof(win[r]), "dyn": hexof(dyn[r]), "gets": got[r]})
            continue
        bufs = [None if k["recv"] is None else k["recv"]["buf"].copy() for k in ranks]

        def view(r):
            return bufs[r][ranks[r]["recv"]["off"]:]

        def sent(r, count, disp=0):
            s = ranks[r]["send"]
            return pack(s["buf"][s["off"]:], s["spec"], count, disp)

        if kind == "gatherv":
            root = op["root"]
            for p in range(n):
                if ranks[p]["send"] is not None:
                    unpack(view(root), sent(p, counts[p]), ranks[root]["recv"]["spec"], counts[p], prefix(counts)[p])
        elif kind == "scatterv":
            root = op["root"]
            for p in range(n):
                unpack(view(p), sent(root, counts[p], prefix(counts)[p]), ranks[p]["recv"]["spec"], counts[p])
        elif kind == "allgatherv":
            for q in range(n):
                for p in range(n):
                    if ranks[p]["send"] is not None:
                        unpack(view(q), sent(p, counts[p]), ranks[q]["recv"]["spec"], counts[p], prefix(counts)[p])
                    elif p != q:  # IN_PLACE: p's contribution is block p of its own receive buffer
                        blk = pack(ranks[p]["recv"]["buf"][ranks[p]["recv"]["off"]:], ranks[p]["recv"]["spec"],
                                   counts[p], prefix(counts)[p])
                        unpack(view(q), blk, ranks[q]["recv"]["spec"], counts[p], prefix(counts)[p])
        else:
            for r in range(n):
                for q in range(n):
                    rc = [counts[p][q] for p in range(n)]
                    unpack(view(q), sent(r, counts[r][q], prefix(counts[r])[q]), ranks[q]["recv"]["spec"], rc[r],
                           prefix(rc)[r])
        for r in range(n):
            recs[r].append({"case": op["name"], "recv": hexof(bufs[r])})
    return recs
