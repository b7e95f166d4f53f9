"""Alltoallw on device buffers: the scenarios as data, and a numpy restatement
of what every buffer must hold afterwards.

`ops(n)` lists the calls of an n-rank run; each one carries every rank's
arguments, so tests/spmd/alltoallw_worker.py executes its own rank's share (on
numpy arrays under MPICH for the fixture, on device tensors under libmpigx)
and `expected(n)` plays all ranks at once.  The fixture
(tests/golden/alltoallw_golden.json) must equal `expected` record for record
(tests/test_alltoallw_cpu.py), which pins both independently of the engine.

A rank's side of a call is one allocation (`buf`, prefilled: the send side
with data, the receive side with a position-dependent sentinel), the byte
offset `off` of the pointer it passes (slack before it; there is slack after
the last block too) and one block per peer: (count, byte displacement, type
spec).  Type specs are strided_cases.py's.

`geometry()` lists the single-process cases of the segmented pack kernel
(copy.hip segw_pack_kernel), `unit_width` restates the engine's choice of a
segment's unit width and `deal` its distribution of blocks."""
import numpy as np

import strided_cases as SC
from strided_cases import BOUNDARY, hexof, size_of, typemap  # noqa: F401

THREADS = 256     # common.hpp kThreads
SEG_GRID = 4096   # typed.hpp kSegGrid
SLACK = 16        # bytes before the pointer (keeps it 16-B aligned) and after the last block
I1, I2, I4, F4, F8, U1 = (np.dtype(x) for x in ("i1", "i2", "i4", "f4", "f8", "u1"))
HOLES = np.dtype([("tag", np.int8), ("val", np.float64)], align=True)  # {int8 @0, float64 @8}: size 9, extent 16
THREE = np.dtype({"names": ["a", "b", "c"], "formats": ["u1", "u2", "i4"], "offsets": [0, 2, 8],
                  "itemsize": 12})  # three runs of 1, 2 and 4 bytes: size 7, extent 12
SPARSE = ("resized", U1, 0, 2)  # one byte out of every two: the smallest type that is not contiguous (W = 1)
PAIRS = ("vector", 2, 2, 4, F8)  # two 16-byte runs 32 bytes apart, extent 48: W = 16 where the addresses allow


# ---------------------------------------------------------------------------
# the type map at byte displacements
# ---------------------------------------------------------------------------
def addrs(spec, count, disp):
    """Byte addresses, in pack order, of `count` instances whose first lies `disp` bytes from the pointer."""
    o, _, ext = typemap(spec)
    return (disp + np.arange(count, dtype=np.int64)[:, None] * ext + o[None, :]).reshape(-1)


def span(spec, count, disp):
    a = addrs(spec, count, disp)
    return (int(a.min()), int(a.max()) + 1) if a.size else (disp, disp)


def contiguous(spec):
    o, _, ext = typemap(spec)
    return ext == len(o) and np.array_equal(o, np.arange(len(o)))


def runs_of(spec):
    """(start, length) of the maximal contiguous byte runs of one instance, in pack order."""
    o = typemap(spec)[0]
    cut = np.flatnonzero(np.diff(o) != 1) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(o)]])
    return [(int(o[s]), int(e - s)) for s, e in zip(starts, ends)]


def unit_width(spec, count, typed_addr, packed_addr):
    """The engine's rule (types.cpp unit_of, per segment): the widest power of
    two up to 16 that divides the type's run offsets, run lengths, strides,
    size and extent, the typed address of the first instance, the packed
    address and the byte length.  A predefined or contiguous type has no run
    table: the addresses and the length alone decide."""
    nbytes = count * size_of(spec)
    if nbytes == 0:
        return 0
    g = typed_addr | packed_addr | nbytes | 16
    if not contiguous(spec):
        g |= typemap(spec)[2] | size_of(spec)
        for start, length in runs_of(spec):
            g |= abs(start) | length
    return g & -g


def deal(units, widths):
    """copy.hip launch_segw_pack: blocks per segment, in proportion to bytes."""
    need = [-(-u // THREADS) for u in units]
    total = sum(u * w for u, w in zip(units, widths))
    G = min(SEG_GRID, sum(need))
    out = []
    for u, w, nd in zip(units, widths, need):
        out.append(0 if u == 0 else max(1, min(nd, int(float(G) * float(u * w) / float(total)))))
    return out


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------
def sentinel(nbytes, seed):
    return ((np.arange(nbytes, dtype=np.int64) * 11 + 17 + 41 * seed) % 239 + 16).astype(np.uint8)


def side(blocks, seed, fill):
    """One rank's side: blocks = [(count, disp, spec)] per peer."""
    hi = max([span(s, c, d)[1] for c, d, s in blocks if c and size_of(s)] + [0])
    lo = min([span(s, c, d)[0] for c, d, s in blocks if c and size_of(s)] + [0])
    assert lo >= -SLACK
    return {"buf": fill(SLACK + hi + SLACK, seed), "off": SLACK, "blocks": blocks}


def call(name, n, send, recv, inplace=False):
    """send[r] / recv[r]: rank r's block list ([q] = towards / from peer q)."""
    ranks = []
    for r in range(n):
        if inplace:  # the receive allocation holds the data that goes out
            ranks.append({"send": None, "recv": side(recv[r], 300 + r, SC.data)})
        else:
            ranks.append({"send": side(send[r], 100 + r, SC.data), "recv": side(recv[r], 200 + r, sentinel)})
    return {"name": name, "inplace": inplace, "ranks": ranks}


def halo(n):
    """A (H + 2) x (W + 2) float64 array with a one-cell ghost frame on a ring:
    the last interior column goes to the right neighbour (a vector, W = 8) and
    the first interior row to the left one (contiguous); they arrive in the
    left ghost column and the bottom ghost row through subarray types.  With
    two ranks both neighbours are one peer, which gets the column only."""
    H, W = 3, 4
    C = W + 2
    col = ("vector", H, 1, C, F8)
    row = ("contig", W, F8)
    ghost_col = ("subarray", (H + 2, C), (H, 1), (1, 0), F8)
    ghost_row = ("subarray", (H + 2, C), (1, W), (H + 1, 1), F8)
    send, recv = [], []
    for r in range(n):
        right, left = (r + 1) % n, (r - 1) % n
        s = [(0, 0, F8)] * n
        v = [(0, 0, F8)] * n
        s[right] = (1, (C + W) * 8, col)
        v[left] = (1, 0, ghost_col)
        if left != right:
            s[left] = (1, (C + 1) * 8, row)
            v[right] = (1, 0, ghost_row)
        send.append(s)
        recv.append(v)
    return call("halo", n, send, recv)


def transpose(n):
    """Rank r holds ROWS[r] x sum(COLS) int32; peer q gets the columns of its
    share, a different subarray per peer, and receives every block contiguously
    at an odd byte displacement."""
    rows = [[3, 2, 4, 1][r % 4] for r in range(n)]
    cols = [[2, 1, 3, 2][q % 4] for q in range(n)]
    C = sum(cols)
    send, recv = [], []
    for r in range(n):
        send.append([(1, 0, ("subarray", (rows[r], C), (rows[r], cols[q]), (0, SC.prefix(cols)[q]), I4))
                     for q in range(n)])
        at, v = 1, []
        for p in range(n):
            v.append((rows[p] * cols[r], at, I4))
            at += rows[p] * cols[r] * 4 + 2  # stays odd
        recv.append(v)
    return call("transpose", n, send, recv)


def mixed_kinds(n):
    """Block kinds by distance (q - r) mod n."""
    kinds = [("contig", 2, F8), I4, HOLES, ("vector", 3, 1, 2, I2)]
    if n == 2:
        kinds = [kinds[0], kinds[2]]
    return [kinds[k % len(kinds)] for k in range(n)]


def mixed(n):
    """Different unit widths in one pack launch: a 16-B-aligned block of 16-byte
    instances (W = 16, 3 instances so that extents step), predefined INT32 at a
    displacement that is 4 mod 8 (W = 4), a struct with holes (two runs, W = 1),
    and with four ranks a vector of int16 (W = 2)."""
    kinds = mixed_kinds(n)
    counts = {0: 3, 1: 5, 2: 2, 3: 2}

    def layout(order):
        at, out = 0, {}
        for k in order:
            spec = kinds[k]
            c = counts[k % 4]
            if isinstance(spec, np.dtype) and spec == I4:
                at = (at + 7) // 8 * 8 + 4
            else:
                at = (at + 15) // 16 * 16
            out[k] = (c, at, spec)
            at = span(spec, c, at)[1] + 1
        return out

    send, recv = [], []
    for r in range(n):
        s, v = layout(range(n)), layout(reversed(range(n)))
        send.append([s[(q - r) % n] for q in range(n)])
        recv.append([v[(r - p) % n] for p in range(n)])
    return call("mixed_widths", n, send, recv)


def plain(n):
    """Every block predefined or contiguous, at odd byte displacements: no pack launch on either side."""
    cnt = [[SC.TAB[(r + 2 * q) % 4] for q in range(n)] for r in range(n)]
    send, recv = [], []
    for r in range(n):
        at, s = 3, []
        for q in range(n):
            s.append((cnt[r][q], at, F4))
            at += cnt[r][q] * 4 + 1
        at, v = 5, []
        for p in range(n):
            v.append((cnt[p][r], at, ("contig", 2, I2)))
            at += cnt[p][r] * 4 + 3
        send.append(s)
        recv.append(v)
    return call("plain", n, send, recv)


def empty_counts(n):
    """[r][q] = instances r sends to q: the last rank sends nothing, rank 1
    receives nothing, rank 1 sends nothing to rank 0."""
    return [[0 if r == n - 1 or q == 1 or (r, q) == (1, 0) else 1 + (r + 2 * q) % 3 for q in range(n)]
            for r in range(n)]


def empties(n):
    cnt = empty_counts(n)
    st, rt = ("vector", 2, 1, 3, I2), ("vector", 2, 1, 2, I2)  # 4 bytes each, neither contiguous
    send, recv = [], []
    for r in range(n):
        send.append([(cnt[r][q], 2 + 40 * q, st) for q in range(n)])
        recv.append([(cnt[p][r], 6 + 28 * p, rt) for p in range(n)])
    return call("empty_segments", n, send, recv)


def inplace(n):
    """IN_PLACE: block q of rank r and block r of rank q hold the same number
    of bytes (kind and count go by r + q), each peer's in a different derived type."""
    kinds = [("vector", 2, 1, 3, I4), ("subarray", (3, 4), (2, 2), (1, 1), I2), BOUNDARY, ("vector", 3, 1, 2, I2),
             HOLES]
    recv = []
    for r in range(n):
        at, v = 0, []
        for q in range(n):
            spec, c = kinds[(r + q) % len(kinds)], 1 + (r + q) % 2
            v.append((c, at, spec))
            at = span(spec, c, at)[1] + 3
        recv.append(v)
    return call("inplace", n, None, recv, inplace=True)


def ops(n):
    return [halo(n), transpose(n), mixed(n), plain(n), empties(n), inplace(n)]


def packs(op, r):
    """Whether rank r's (send, receive) side goes through the pack kernel."""
    def one(s):
        return s is not None and any(c and size_of(t) and not contiguous(t) for c, _, t in s["blocks"])
    me = op["ranks"][r]
    return one(me["recv"] if op["inplace"] else me["send"]), one(me["recv"])


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def play(op):
    """[rank] -> record of one call, as alltoallw_worker.py writes it."""
    ranks = op["ranks"]
    n = len(ranks)
    out = [k["recv"]["buf"].copy() for k in ranks]
    for r in range(n):
        src = ranks[r]["recv"] if op["inplace"] else ranks[r]["send"]
        for q in range(n):
            c, d, t = src["blocks"][q]
            stream = src["buf"][addrs(t, c, src["off"] + d)]
            c2, d2, t2 = ranks[q]["recv"]["blocks"][r]
            a = addrs(t2, c2, ranks[q]["recv"]["off"] + d2)
            assert len(a) == len(stream), (op["name"], r, q, len(a), len(stream))
            out[q][a] = stream
    return [{"case": op["name"], "recv": hexof(out[r]), "send_unchanged": True} for r in range(n)]


def expected(n):
    """[rank][op] -> record."""
    played = [play(op) for op in ops(n)]
    return [[p[r] for p in played] for r in range(n)]


def rounds(n, stage=4096):
    """One typed call whose blocks span at least three staging rounds of an
    arena of `stage` bytes (mpigx.cpp vexchange: R = (stage - 256) / n rounded
    down to 16), ragged, out of PAIRS into SPARSE.  Model-checked only."""
    R = (stage - 256) // n // 16 * 16
    cnt = [[-(-3 * R // 32) + 13 * ((r + 2 * q) % 3) + 1 for q in range(n)] for r in range(n)]
    send, recv = [], []
    for r in range(n):
        at, s = 0, []
        for q in range(n):
            s.append((cnt[r][q], at, PAIRS))
            at += cnt[r][q] * 48 + 16
        at, v = 1, []
        for p in range(n):
            v.append((cnt[p][r] * 32, at, SPARSE))
            at += cnt[p][r] * 64 + 5
        send.append(s)
        recv.append(v)
    return call("rounds", n, send, recv)


# ---------------------------------------------------------------------------
# kernel geometry (one process, the diagnostic entry point, model only)
# ---------------------------------------------------------------------------
def geo(name, segs, base=0, want_w=None):
    """segs = [(spec, count, byte displacement, packed offset)]; `base` = bytes
    by which the typed pointer is moved off its 16-B alignment."""
    return {"name": name, "segs": segs, "base": base, "want_w": want_w}


def geometry():
    out = []
    # unit counts 0, 1, 255, 256, 257, 513 (W = 1: one unit per instance of SPARSE)
    at, pk, segs = 0, 0, []
    for c in (0, 1, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1):
        segs.append((SPARSE, c, at, pk))
        at += 2 * c + 6
        pk += (c + 15) // 16 * 16
    out.append(geo("unit_counts", segs, want_w=[0, 1, 1, 1, 1, 1]))
    # past the 4096-block deal: just over 1 MiB of W = 1 units beside a 3-unit segment
    big = SEG_GRID * THREADS + 77
    out.append(geo("past_the_grid", [(SPARSE, 3, 0, 0), (SPARSE, big, 16, 16)], want_w=[1, 1]))
    # W = 16 and W = 1 segments of equal byte length in one launch
    out.append(geo("w16_beside_w1", [(PAIRS, 8, 0, 0), (SPARSE, 256, 8 * 48, 256)], want_w=[16, 1]))
    # a 3-run type (the run search) whose 7-byte instances straddle the blocks' share boundaries
    out.append(geo("three_runs_straddle", [(THREE, 101, 0, 0)], want_w=[1]))
    # the same type at typed addresses that are 0, 8, 4, 2 and 1 mod 16
    segs = [(PAIRS, 3, 160 * j + d, 96 * j) for j, d in enumerate((0, 8, 4, 2, 1))]
    out.append(geo("typed_base_lowers_w", segs, want_w=[16, 8, 4, 2, 1]))
    # the pointer itself off alignment: every segment drops to bytes
    out.append(geo("odd_pointer", [(PAIRS, 3, 0, 0), (F8, 4, 160, 96)], base=1, want_w=[1, 1]))
    return out


def geometry_buffers(g):
    """(typed, packed) allocations of a geometry case, the typed pointer's offset, and the two sizes."""
    hi = max(span(t, c, d)[1] for t, c, d, _ in g["segs"] if c)
    pk = max(o + c * size_of(t) for t, c, _, o in g["segs"])
    return SLACK + g["base"] + hi + SLACK, SLACK + g["base"], pk + SLACK


def geometry_expected(g, typed, packed, unpack):
    """What the written buffer holds afterwards (the other one is unchanged)."""
    _, off, _ = geometry_buffers(g)
    out = (typed if unpack else packed).copy()
    for t, c, d, o in g["segs"]:
        a = addrs(t, c, off + d)
        p = o + np.arange(len(a), dtype=np.int64)
        if unpack:
            out[a] = packed[p]
        else:
            out[p] = typed[a]
    return out
