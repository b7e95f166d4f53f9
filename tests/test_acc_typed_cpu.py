"""Accumulate / Get_accumulate through non-contiguous derived datatypes, the
parts that need no GPU: the case table and model of
tests/spmd/acc_typed_cases.py against the recorded MPICH run
(tests/golden/acc_typed_golden.json), the claims the table makes about
acc_typed_kernel's loop regions and the Get_accumulate chunk seams (restated
here from the launch arithmetic, not assumed), the built kernels' private
segments, and the mirror's arguments."""
import glob
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "spmd"))
sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))
import acc_typed_cases as C  # noqa: E402
from test_kernel_resources_cpu import BUILD, LLVM, OBJS, REPS, _kernel_private_sizes  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "acc_typed_golden.json")))
BY_ID = {c["id"]: c for c in C.CASES}


def test_model_reproduces_every_recorded_mpich_case():
    n = GOLDEN["n"]
    assert n == C.N and len(GOLDEN["records"]) == n
    want_ids = [c["id"] for c in C.CASES if c["mpich"]]
    for rank, recs in enumerate(GOLDEN["records"]):
        assert [r["case"] for r in recs] == want_ids  # every MPICH-expressible case, nothing else
        lengths = {t: C.window_elems(t) for t in {c["type"] for c in C.CASES}}
        for r in recs:
            c = BY_ID[r["case"]]
            length = c["wlen"] if c["dyn"] else lengths[c["type"]]
            win, res = C.model(c, rank, n, length)
            assert all(rc == 0 for rc in r["rc"]), (c["id"], r["rc"])
            assert r["window"] == C.enc(win), (c["id"], rank, "window")
            assert r["result"] == (C.enc(res) if res is not None else None), (c["id"], rank, "result")
            posts = 2 if c["shape"] == "order" else 1
            assert r["origin"] == [C.enc(C.origin_buffer(c, rank, j)) for j in range(posts)], (c["id"], rank, "origin")


@pytest.mark.parametrize("c", C.CASES, ids=[c["id"] for c in C.CASES])
def test_every_case_would_expose_a_wrong_kernel(c):
    """The model's window differs from the initial one (NO_OP: the fetched
    values differ from the untouched result buffer) and from the window that
    the same elements applied at CONTIGUOUS offsets give; every byte outside
    the target map keeps the sentinel; the result differs from one gathered at
    contiguous offsets."""
    n, es = C.N, C.esize(c["type"])
    me = 0 if c["shape"] == "multi" else 1
    init = C.window_init(c, me, n)
    win, res = C.model(c, me, n)
    same = lambda a, b: np.array_equal(a.view(np.uint8), b.view(np.uint8))  # noqa: E731
    toff = C.stream_offsets(c["t"], es)
    assert toff.size == c["count"] == np.unique(toff).size  # the map does not overlap itself
    one = c["count"] == 1  # a single element has no layout to get wrong: it is there for the loop region
    assert one or not np.array_equal(toff, np.arange(toff.size))  # the map is not contiguous
    if c["op"] != "NO_OP":
        assert not same(win, init)
        flat, _ = C.model(c, me, n, offsets=np.arange(c["count"], dtype=np.int64))
        assert one or not same(win, flat)
    else:
        assert same(win, init)
    touched = np.zeros(win.size, bool)
    for j in range(2 if c["shape"] == "order" else 1):
        touched[c["disp"] + j * C.ORDER_SHIFT + toff] = True
    outside = np.repeat(~touched, es)
    assert (win.view(np.uint8)[outside] == C.SENTINEL).all() and outside.any()
    if c["kind"] == "gacc":
        assert not same(res, C.result_buffer(c))
        roff = C.stream_offsets(c["r"], es)
        out = np.ones(res.size, bool)
        out[roff] = False
        assert (res.view(np.uint8)[np.repeat(out, es)] == C.SENTINEL).all()
        # gathered at contiguous window offsets instead of through the target map
        wrong = C.window_init(c, (me + 1) % n, n)[c["disp"]:c["disp"] + c["count"]]
        assert not same(res[roff], wrong)
    # origin side: the operand sits in the map, the rest is sentinel
    ob = C.origin_buffer(c, me)
    oout = np.ones(ob.size, bool)
    oout[C.stream_offsets(c["o"], es)] = False
    assert (ob.view(np.uint8)[np.repeat(oout, es)] == C.SENTINEL).all()


# --- acc_typed_kernel's launch arithmetic, restated ---------------------------
def regions(count):
    """rma.cpp apply_one: g = clamp(ceil(count / (kAccTypedU * 256)), 1,
    kAccTypedGridCap) blocks of 256; acc_typed_kernel: `for (; i + 3 nt < n;
    i += 4 nt)` then `for (; i < n; i += nt)`."""
    g = max(1, min(-(-count // 1024), 1024))
    nt = 256 * g
    main = tail = 0
    for t in range(0, nt, max(1, nt // 512)) if nt > 4096 else range(nt):
        i = t
        while i + 3 * nt < count:
            i, main = i + 4 * nt, main + 1
        tail += len(range(i, count, nt))
    return {"g": g, "nt": nt, "main": main, "tail": tail, "capped": -(-count // 1024) > 1024}


def test_geometry_constants_are_the_engines():
    src = open(os.path.join(ROOT, "mpi.jl_amd", "csrc", "common.hpp")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (kAccTypedU|kAccTypedGridCap|kAccTypedRuns|kThreads) = (\d+);", src)}
    assert consts == {"kAccTypedU": C.U, "kAccTypedGridCap": C.GRID_CAP, "kAccTypedRuns": C.RUN_CAP, "kThreads": C.THREADS}
    rt = open(os.path.join(ROOT, "mpi.jl_amd", "csrc", "runtime.hpp")).read()
    assert int(re.search(r"constexpr int kRmaRunCap = (\d+);", rt).group(1)) == C.RUN_CAP
    for count in (1, 100, 700, 1000, 1024, 4099, (1 << 20) + 5):
        g, r = C.geometry(count), regions(count)
        assert (g["g"], g["nt"], g["capped"]) == (r["g"], r["nt"], r["capped"])
        if r["nt"] <= 4096:
            assert (g["main_elems"], g["tail_elems"]) == (4 * r["main"], r["tail"])


def test_table_reaches_every_loop_region():
    acc = {c["id"]: regions(c["count"]) for c in C.CASES if c["kind"] == "acc" and c["shape"] == "one"}
    counts = {c["id"]: c["count"] for c in C.CASES}
    assert counts["1 element"] == 1 and acc["1 element"]["main"] == 0
    few = [k for k, r in acc.items() if 1 < counts[k] < C.THREADS and r["g"] == 1]
    assert few  # fewer elements than one block
    r = acc["tail only x700"]
    assert r["main"] == 0 and r["tail"] == 700 and counts["tail only x700"] > 2 * C.THREADS  # several tail strides
    r = acc["body and tail x1000"]
    assert r["main"] > 0 and r["tail"] > 0 and 4 * r["main"] + r["tail"] == 1000
    cap = BY_ID["past the grid cap"]
    g = C.geometry(cap["count"])
    assert g["capped"] and g["g"] == C.GRID_CAP and g["main_elems"] > 0 and g["tail_elems"] > 0
    assert g["main_elems"] >= C.U * g["nt"]  # a whole grid-wide main iteration
    assert C.esize(cap["type"]) <= 2 and cap["wlen"] * C.esize(cap["type"]) < (3 << 19)  # about a megabyte


def test_table_covers_sizes_ops_and_layouts():
    assert {C.esize(c["type"]) for c in C.CASES} == {1, 2, 4, 8, 16}
    types = {c["type"] for c in C.CASES}
    assert {"complex128", "bfloat16"} <= types
    assert all(c["mpich"] == (c["type"] != "bfloat16") for c in C.CASES)
    ops = {(c["op"], np.dtype(C.npdt(c["type"])).kind if c["type"] != "bfloat16" else "f") for c in C.CASES}
    assert ("SUM", "f") in ops and ("MAX", "i") in ops and ("BXOR", "i") in ops
    assert any(c["op"] == "REPLACE" for c in C.CASES)
    assert any(c["op"] == "NO_OP" and c["kind"] == "gacc" for c in C.CASES)
    k = lambda s: s[0]["k"]  # noqa: E731
    assert any(k(c["o"]) == "contig" and k(c["t"]) == "vector" for c in C.CASES)
    assert any(k(c["o"]) == "subarray" and k(c["t"]) == "subarray" and c["o"] != c["t"] and c["r"] and
               k(c["r"]) not in ("contig", "subarray") for c in C.CASES)
    rz = [c for c in C.CASES if k(c["t"]) == "resized" and c["t"][1] > 1]
    assert rz
    for c in rz:  # instances interleave: instance 1 starts inside instance 0's span
        off = C.stream_offsets(c["t"], C.esize(c["type"]))
        m = C.instance_elems(c["t"], C.esize(c["type"]))
        assert off[m] < off[:m].max()
    st = [c for c in C.CASES if k(c["t"]) == "struct" and C.nruns(c["t"][0]) >= 3]
    assert any(len(set(c["t"][0]["bl"])) >= 3 for c in st)  # unequal runs: the binary search takes both branches
    assert any(C.nruns(c["t"][0]) == C.RUN_CAP for c in C.CASES)
    for c in C.CASES:  # what nruns() counts is what the engine flattens: no two adjacent or equal-length neighbours
        if k(c["t"]) == "struct":
            bl, d = c["t"][0]["bl"], c["t"][0]["disp_el"]
            assert all(d[i] + bl[i] < d[i + 1] for i in range(len(bl) - 1))
            assert all(bl[i] != bl[i + 1] for i in range(len(bl) - 1))
    assert sum(c["dyn"] for c in C.CASES) == 1
    assert {c["shape"] for c in C.CASES} == {"one", "order", "multi"}
    order = next(c for c in C.CASES if c["shape"] == "order")
    toff = C.stream_offsets(order["t"], C.esize(order["type"]))
    assert order["op"] == "REPLACE+SUM" and set(toff) & set(toff + C.ORDER_SHIFT)  # the two posts overlap
    multi = next(c for c in C.CASES if c["shape"] == "multi")
    assert multi["op"] == "SUM" and C.npdt(multi["type"]).kind == "i"


def test_chunk_seams_fall_inside_runs_and_instances():
    inside_run = inside_instance = 0
    for tname, tag in (("float32", "seam4"), ("int64", "seam8")):
        per = C.per_of(tname)
        assert per == max(256, (C.SCRATCH // C.N) & ~255) // C.esize(tname)  # rma.cpp win_setup / acc_common
        cs = [c for c in C.CASES if c["id"].startswith(tag)]
        assert sorted(c["count"] for c in cs) == [per - 1, per, per + 1, 3 * per + 7]
        for c in cs:
            es = C.esize(tname)
            assert c["kind"] == "gacc" and c["per"] == per and c["t"][0]["k"] != "contig"
            starts, m = C.run_starts(c["t"], es), C.instance_elems(c["t"], es)
            for s in C.seams(c["count"], per):
                inside_run += s not in starts
                inside_instance += c["t"][1] > 1 and s % m != 0
        assert len(C.seams(3 * per + 7, per)) == 3 and not C.seams(per, per) and C.seams(per + 1, per) == [per]
    assert inside_run >= 2 and inside_instance >= 1
    assert any(c["r"][0]["k"] != "contig" for c in C.CASES if c["id"].startswith("seam"))  # chunks into a typed result


def test_refusal_list_is_the_issues():
    assert [r["id"] for r in C.REFUSALS] == ["mixed-basic struct", "basic-type mismatch", "element-count mismatch",
                                             "65-run target", "hvector of FLOAT, 6-byte stride",
                                             "span leaves the window"]
    assert [r["want"] for r in C.REFUSALS] == [C.MPI_ERR_TYPE] * 5 + [C.MPI_ERR_RMA_RANGE]
    r65 = C.REFUSALS[3]["t"][0]
    assert C.nruns(r65) == C.RUN_CAP + 1 and sum(r65["bl"]) == C.REFUSALS[3]["o"][1]
    cm = C.REFUSALS[2]
    assert C.stream_offsets(cm["t"], 4).size != cm["o"][1]


# --- the built kernels ---------------------------------------------------------
@pytest.mark.skipif(not OBJS or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="kernel objects not built (run __graft_entry__.build())")
@pytest.mark.parametrize("rep", REPS)
def test_acc_typed_kernels_exist_without_private_segment(rep, tmp_path):
    sizes = {}
    for obj in sorted(glob.glob(os.path.join(BUILD, f"kern_{rep}_p*.o"))):
        sizes.update(_kernel_private_sizes(obj, str(tmp_path)))
    typed = {k: v for k, v in sizes.items() if "16acc_typed_kernel" in k}
    assert len(typed) >= 2, f"acc_typed_kernel instantiations missing for {rep}"  # REPLACE and NO_OP at the least
    assert any("OpReplace" in k for k in typed) and any("OpNoop" in k for k in typed)
    assert all(v == 0 for v in typed.values()), {k: v for k, v in typed.items() if v}


# --- the mirror ------------------------------------------------------------------
def test_mirror_takes_buffers_and_target():
    from mpigx import rma
    for fn in (rma.Accumulate, rma.Get_accumulate):
        p = inspect.signature(fn).parameters
        assert "target" in p and p["target"].default is None
    assert list(inspect.signature(rma.Accumulate).parameters)[:6] == ["origin_buffer", "count", "target_rank",
                                                                      "target_disp", "op", "win"]
    assert list(inspect.signature(rma.Get_accumulate).parameters)[:7] == ["origin_buffer", "result_buffer", "count",
                                                                          "target_rank", "target_disp", "op", "win"]
    from mpigx.api import Buffer, Datatype, FLOAT
    vec = Datatype(0x7B000001, "vector(test)", host_val=0x8C000001)  # handles as Types.create_vector returns them
    o = Buffer(np.zeros(8, np.float32), 2, vec)
    r = Buffer(np.zeros(9, np.float32), 3, FLOAT)
    # an MPI.Buffer goes by its own count and datatype, an array by `count` and its element type
    assert rma._acc_sides(o, r, None, None) == ((2, vec.val, vec.host), (3, FLOAT.val, FLOAT.host), (2, vec.val, vec.host))
    assert rma._acc_sides(o, None, None, (5, FLOAT)) == ((2, vec.val, vec.host), None, (5, FLOAT.val, FLOAT.host))
    assert rma._acc_sides(np.zeros(8, np.float32), None, 6, Buffer(None, 1, vec)) == (
        (6, FLOAT.val, FLOAT.host), None, (1, vec.val, vec.host))
    # today's form: count and the origin's element type on every side
    assert rma._acc_sides(np.zeros(8, np.float32), np.zeros(8, np.float32), 7, None) == (
        ((7, FLOAT.val, FLOAT.host),) * 3)
