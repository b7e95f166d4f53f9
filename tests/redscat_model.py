"""CPU restatement of MPICH 3.3.2's MPI_Reduce_scatter_block / MPI_Reduce_scatter
for the built-in (commutative) ops, bit for bit, and the seeded inputs of the
fixtures recorded from MPICH (tests/golden/gen_redscat_golden.c, the same
splitmix64 keying and gen modes as gen_mpich_golden.c).

Which algorithm: `total` = (sum of all ranks' receive counts) x element size;
below `switch` (524288) bytes recursive halving, from it up pairwise exchange.

Recursive halving: pof2 = largest power of two <= n, rem = n - pof2.  Pre-step:
y[j] = op(inout = x[2j+1], in = x[2j]) for j < rem, y[j] = x[j+rem] otherwise.
The block of real rank r is folded at new rank d = r // 2 if r < 2 rem else
r - rem, as T(d, log2 pof2) with T(q, 0) = y[q] and
T(q, j) = op(inout = T(q, j-1), in = T(q ^ (pof2 >> j), j-1)).

Pairwise exchange: acc = x[r]; acc = op(inout = acc, in = x[(r - i) mod n]) for
i = 1 .. n-1.
"""
import numpy as np

from oracle.mpich_model import DTYPES, OPS, apply_op, fold_linear  # noqa: F401

SWITCH = 524288


def _pof2(n):
    p = 1
    while p * 2 <= n:
        p *= 2
    return p


def _halving(blocks, r, dtname, opname, swap=False):
    """blocks[q] = rank q's copy of rank r's block."""
    n = len(blocks)
    pof2 = _pof2(n)
    rem = n - pof2

    def op(inout, inv):
        return apply_op(opname, dtname, inv.copy(), inout) if swap else apply_op(opname, dtname, inout.copy(), inv)

    y = [op(blocks[2 * j + 1], blocks[2 * j]) if j < rem else blocks[j + rem] for j in range(pof2)]
    d = r // 2 if r < 2 * rem else r - rem
    lg = pof2.bit_length() - 1

    def T(q, j):
        if j == 0:
            return y[q]
        return op(T(q, j - 1), T(q ^ (pof2 >> j), j - 1))

    return T(d, lg).copy()


def _pairwise(blocks, r, dtname, opname, swap=False):
    n = len(blocks)
    acc = blocks[r].copy()
    for i in range(1, n):
        x = blocks[(r - i) % n]
        acc = apply_op(opname, dtname, x.copy(), acc) if swap else apply_op(opname, dtname, acc, x)
    return acc


def reduce_scatter(inputs, counts, dtname, opname, switch=SWITCH, order="mpich", swap=False):
    """Per-rank outputs.  inputs[q]: rank q's sendbuf of sum(counts) elements.
    order "linear": the rank-ordered left fold of each block (MPIGX_ORDER_LINEAR).
    swap=True exchanges the operand roles of every op (the discrimination
    check of the fixtures, never the model of anything)."""
    n = len(inputs)
    assert len(counts) == n
    total = int(sum(counts)) * np.dtype(DTYPES[dtname][1]).itemsize
    out, at = [], 0
    for r in range(n):
        blocks = [np.ascontiguousarray(x[at:at + counts[r]]) for x in inputs]
        at += counts[r]
        if n == 1 or counts[r] == 0:
            out.append(blocks[r].copy())
        elif order == "linear":
            out.append(fold_linear(blocks, dtname, opname))
        elif total < switch:
            out.append(_halving(blocks, r, dtname, opname, swap))
        else:
            out.append(_pairwise(blocks, r, dtname, opname, swap))
    return out


# ---------------------------------------------------------------------------
# inputs of the fixtures: gen_redscat_golden.c gen(), element i of rank `rank`
# ---------------------------------------------------------------------------
G_RAND, G_LOGIC, G_NAN, G_SZERO, G_EDGE, G_WIDE = 0, 1, 3, 4, 6, 7


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _uf32(r):
    return ((r >> np.uint64(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23)


def _uf64(r):
    return ((r >> np.uint64(11)).astype(np.int64) - (1 << 52)).astype(np.float64) / 4503599627370496.0


def gen_input(dtname, count, rank, nranks, seed, mode):
    npdt = np.dtype(DTYPES[dtname][1])
    kind = DTYPES[dtname][2]
    i = np.arange(count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = np.uint64(seed) * np.uint64(0x100000001B3) ^ (np.uint64(rank) << np.uint64(40))
    r = _splitmix64(base ^ i)
    ii = i.astype(np.int64)
    if kind in ("int", "uint", "byte"):
        v = r.copy()
        if mode == G_LOGIC:
            v[(r & np.uint64(0xFF)) < 90] = 0
        return v.astype(np.dtype(f"u{npdt.itemsize}")).view(npdt)  # low bytes
    if kind == "float":
        uf = _uf32 if npdt.itemsize == 4 else _uf64
        v = uf(r)
        if mode == G_WIDE:
            v = np.ldexp(v, (r & np.uint64(31)).astype(np.int32) - 16)
        if mode == G_NAN:
            v = (np.float64(rank + 1) * (1 + ii % 3)).astype(npdt)
            if rank == seed % nranks:
                v[ii % 2 == 0] = np.nan
        elif mode == G_SZERO:
            v = np.full(count, -0.0 if rank % 2 else 0.0, dtype=npdt)
        elif mode == G_EDGE:
            k = (rank + ii) % 6
            tiny, huge = (1e-45, 3.4e38) if npdt.itemsize == 4 else (5e-324, 1.7e308)
            table = np.array([np.inf, -np.inf, tiny, -0.0, huge], dtype=npdt)
            v = v.astype(npdt)
            m = k < 5
            v[m] = table[k[m]]
        return v.astype(npdt)
    if kind == "complex":
        uf = _uf32 if npdt.itemsize == 8 else _uf64
        out = np.empty(count, dtype=npdt)
        out.real = uf(r)
        out.imag = uf(_splitmix64(r))
        return out
    raise KeyError(dtname)


def counts_of(case, n):
    """Receive counts of a fixture case: the block form, or base + (q % 3) - 1."""
    if case["v"]:
        return [max(0, case["count"] + (q % 3) - 1) for q in range(n)]
    return [case["count"]] * n


def case_inputs(case):
    n = case["n"]
    total = sum(counts_of(case, n))
    return [gen_input(case["dtype"], total, q, n, case["seed"], case["mode"]) for q in range(n)]


# the recorded outputs, split by world size (tests/golden/pack_redscat_golden.py)
GOLDEN_FILES = (("redscat_golden.npz", (1, 2, 3, 4, 5)), ("redscat_golden_n6_n8.npz", (6, 8)),
                ("redscat_golden_n7.npz", (7,)))


def load_golden():
    """(cases, {case id: uint8 array}) of the fixtures recorded from MPICH."""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "redscat_golden_manifest.json")) as f:
        cases = json.load(f)
    arrays = {}
    for name, _ in GOLDEN_FILES:
        with np.load(os.path.join(here, name), allow_pickle=False) as z:
            arrays.update({k: z[k] for k in z.files})
    return cases, arrays


def spans_of(case, mine):
    """Element spans of a rank's output that the fixture holds."""
    if case["spans"] and mine > 512:
        return [(0, 256), (mine - 256, mine)]
    return [(0, mine)]


def sample(x, case):
    return np.concatenate([x[lo:hi] for lo, hi in spans_of(case, x.size)]) if x.size else x


def split_outputs(case, blob):
    """The fixture's array of a case (uint8, ranks concatenated) -> per-rank typed samples."""
    npdt = np.dtype(DTYPES[case["dtype"]][1])
    out, at = [], 0
    for c in counts_of(case, case["n"]):
        k = sum(hi - lo for lo, hi in spans_of(case, c)) * npdt.itemsize
        out.append(np.ascontiguousarray(blob[at:at + k]).view(npdt))
        at += k
    assert at == blob.size
    return out
