"""The RMA data-path plan (tests/spmd/rma_data_cases.py) reaches what it
claims to reach.  The launch arithmetic of the three device paths is restated
here in a few lines; if rma.cpp, acc_kernel, xfer_kernel or block_copy change
theirs, these assertions fail and the counts get chosen again.  And every
accumulate case's model output would expose a wrong kernel: the op changes
the window, the MIN / MAX operand roles are visible, and an origin read one
element off gives a different result."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "spmd"))
import rma_data_cases as C  # noqa: E402
from golden_io import same_bits  # noqa: E402


# --- the launch arithmetic, restated -----------------------------------------
def acc_regions(count):
    """rma.cpp apply_one: g = clamp(ceil(count / (4 * 256)), 1, 1024) blocks of
    256; acc_kernel: `for (; i + 3 nt < n; i += 4 nt)` then `for (; i < n; i += nt)`."""
    g = max(1, min(-(-count // 1024), 1024))
    nt = 256 * g
    main_iters, tail = [], 0
    for t in (0, nt - 1):  # the first and the last thread of the grid
        i, k = t, 0
        while i + 3 * nt < count:
            i, k = i + 4 * nt, k + 1
        main_iters.append(k)
        tail = max(tail, len(range(i, count, nt)))
    idle = max(0, nt - count)
    return {"g": g, "nt": nt, "main_first": main_iters[0], "main_last": main_iters[1], "tail_strides": tail,
            "idle": idle, "capped": -(-count // 1024) > 1024}


def copy_path(nbytes, dst_mod, src_mod):
    """rma.cpp apply_one / pull: g = clamp(ceil(bytes / 64 Ki), 1, 256);
    xfer_kernel: slice = ceil(bytes / g) rounded up to 16; block_copy: 16-B
    vectors when dst = src (mod 16), 4-B words when dst = src (mod 4), else bytes."""
    want = -(-nbytes // 65536)
    g = max(1, min(want, 256))
    x = (dst_mod - src_mod) % 16
    branch = "vec16" if x == 0 else "word4" if x % 4 == 0 else "byte"
    head = {"vec16": -dst_mod % 16, "word4": -dst_mod % 4, "byte": 0}[branch]
    return {"g": g, "branch": branch, "head": min(head, nbytes), "capped": want > 256,
            "slice": (-(-nbytes // g) + 15) // 16 * 16}


def test_model_geometry_agrees_with_the_restatement():
    for count in C.ACC_COUNTS + [2, 256, 257, 1023, 2048, 5000, (1 << 20) + 1]:
        a, b = C.acc_geometry(count), acc_regions(count)
        assert (a["g"], a["nt"], a["capped"]) == (b["g"], b["nt"], b["capped"]), count
        assert a["main_iters"] == b["main_first"], count
        assert a["main_elems"] + a["tail_elems"] == count
    for nb in C.BYTE_SIZES:
        for d, m in C.byte_aligns(nb):
            a, b = C.copy_geometry(nb, m, (m - d) % 16), copy_path(nb, m, (m - d) % 16)
            assert (a["g"], a["branch"], a["head"], a["capped"], a["slice"]) == \
                (b["g"], b["branch"], b["head"], b["capped"], b["slice"]), (nb, d, m)


def test_accumulate_counts_reach_every_loop_region():
    reg = {c: acc_regions(c) for c in C.ACC_COUNTS}
    assert reg[1]["g"] == 1 and reg[1]["idle"] == 255
    assert reg[255]["main_first"] == 0 and reg[255]["idle"] == 1
    # main only: one block, every thread one main iteration, nothing left
    assert reg[1024] == dict(reg[1024], g=1, main_first=1, main_last=1, tail_strides=0)
    # tail only, more than one block, some threads idle in the last stride
    assert reg[1025] == dict(reg[1025], g=2, main_first=0, main_last=0, tail_strides=3)
    assert 1025 % reg[1025]["nt"] != 0
    # main and tail in one launch: the first 259 threads take the main loop
    r = reg[4099]
    assert r["g"] == 5 and r["main_first"] == 1 and r["main_last"] == 0 and r["tail_strides"] == 3
    assert C.acc_geometry(4099)["main_threads"] == 259
    # the grid at its cap: main loop exactly once / twice plus a ragged tail
    r = reg[1 << 20]
    assert r["g"] == 1024 and r["main_first"] == r["main_last"] == 1 and r["tail_strides"] == 0 and not r["capped"]
    r = reg[(2 << 20) + 517]
    assert r["g"] == 1024 and r["capped"] and r["main_first"] == r["main_last"] == 2 and r["tail_strides"] == 1
    assert C.acc_geometry((2 << 20) + 517)["tail_elems"] == 517
    # the matrix runs tail only, main only and main plus tail; the capped counts run for every element size
    assert C.MATRIX_COUNTS == [1024, 1025, 4099]
    planned = {(c["type"], c["count"], c["kind"]) for ep in C.plan_matrix() for c in ep["cases"]}
    for t in C.TYPES:
        for cnt in C.MATRIX_COUNTS:
            assert (t, cnt, "acc") in planned and (t, cnt, "gacc") in planned
    assert sorted(C.esize(t) for t in C.SIZE_TYPES) == [1, 2, 4, 8, 16]
    for t in C.SIZE_TYPES:
        for cnt in C.CAPPED_COUNTS + C.SMALL_COUNTS:
            assert (t, cnt, "acc") in planned
        ops = {c["op"] for ep in C.plan_matrix() for c in ep["cases"] if c["type"] == t and c["count"] == 1 << 20}
        assert "SUM" in ops and ("MAX" in ops or not C.valid("MAX", t))


def test_byte_plan_reaches_every_copy_branch():
    seen = set()
    for ep in C.plan_bytes():
        for c in ep["cases"]:
            p = copy_path(c["nbytes"], c["dst_mod"], c["src_mod"])
            assert c["delta"] == (c["dst_mod"] - c["src_mod"]) % 16
            seen.add((c["kind"], ep["sync"], p["branch"], p["head"] > 0, p["g"] > 1, p["capped"]))
            seen.add((c["kind"], ep["sync"], c["nbytes"]))
    for kind in ("put", "get"):
        for sync in ("fence", "lock"):
            for nb in C.BYTE_SIZES:
                assert (kind, sync, nb) in seen
            for branch in ("vec16", "word4", "byte"):
                heads = (True, False) if branch != "byte" else (False,)
                for head in heads:
                    for blocks in (False, True):  # one block / more than one
                        assert (kind, sync, branch, head, blocks, False) in seen, (kind, sync, branch, head, blocks)
            # past the 256-block cap: the vector branch with a head, and the 4-B branch
            assert (kind, sync, "vec16", True, True, True) in seen and (kind, sync, "word4", False, True, True) in seen
    # two blocks whose slice is rounded up to 16 B: the second block starts on a 16-B multiple past bytes / 2
    p = copy_path(65537, 0, 0)
    assert p["g"] == 2 and p["slice"] == 32784 and p["slice"] * 2 > 65537
    assert copy_path(65535, 0, 0)["g"] == 1 and copy_path(3 * 65536 + 5, 0, 0)["g"] == 4
    assert copy_path((16 << 20) + 19, 0, 0) == dict(copy_path((16 << 20) + 19, 0, 0), g=256, capped=True)


def test_seam_counts_sit_on_the_chunk_boundary():
    for n in (2, 3):
        for ep in C.plan_seams(n):
            for c in ep["cases"]:
                if c["kind"] != "gacc":
                    continue
                slot = max(256, (C.SEAM_SCRATCH // n) & ~255)  # rma.cpp win_setup
                assert c["per"] == slot // C.esize(c["type"]) and slot == {2: 2048, 3: 1280}[n]
            counts = sorted(c["count"] - c["per"] for c in ep["cases"] if c["kind"] == "gacc")
            if counts:
                per = ep["cases"][0]["per"]
                assert counts == [-1, 0, 1, 2 * per + 7]
    ops = {(c["type"], c["op"]) for ep in C.plan_seams(3) for c in ep["cases"] if c["kind"] == "gacc"}
    assert ops == {(t, op) for t in C.SIZE_TYPES for op in ("SUM", "REPLACE", "NO_OP")}
    assert {c["type"] for ep in C.plan_seams(3) for c in ep["cases"] if c["kind"] == "fop"} == {"bfloat16", "complex128"}


def test_order_epochs_wrap_the_envelope_ring_and_overlap():
    assert C.ORDER_POSTS > 2 * 16 and C.MULTI_POSTS > 16  # kRmaSlots = 16
    s = C.order_starts()
    assert max(s) + C.ORDER_COUNT <= 1025 + C.ORDER_COUNT and len(set(s)) == len(s)
    assert all(abs(a - b) < C.ORDER_COUNT for a, b in zip(s, s[1:]))  # consecutive ranges overlap
    assert acc_regions(C.ORDER_COUNT)["g"] > 1
    # the op sequence does not commute: applying it backwards gives another window
    for t in ("float32", "int64"):
        w0 = np.arange(C.ORDER_COUNT + 1025).astype(C.npdt(t))
        fwd, bwd = w0.copy(), w0.copy()
        order = list(range(C.ORDER_POSTS))
        for out, seq in ((fwd, order), (bwd, order[::-1])):
            for j in seq:
                op, o = C.order_operand(t, j, 5)
                out[s[j]:s[j] + C.ORDER_COUNT] = C.model(t, out[s[j]:s[j] + C.ORDER_COUNT].copy(), o, op)[0]
        assert not np.array_equal(fwd, bwd)
        assert {C.order_operand(t, j, 5)[0] for j in order} == set(C.ORDER_OPS[t])


def _acc_cases():
    seen = set()
    for eps in (C.plan_matrix(), C.plan_seams(2), C.plan_seams(3)):
        for ep in eps:
            for c in ep["cases"]:
                key = (c["type"], c["op"], c["count"])
                if key not in seen:
                    seen.add(key)
                    yield c


def test_every_accumulate_case_would_expose_a_wrong_kernel():
    n = 0
    for c in _acc_cases():
        t, op, cnt = c["type"], c["op"], c["count"]
        bf = t == "bfloat16"
        w, o = C.operand_pair(t, op, cnt, 7)
        new, old = C.model(t, w, o[:cnt], op)
        assert same_bits(old, w, bf16=bf)
        if op == "NO_OP":
            assert same_bits(new, w, bf16=bf)
            continue
        # strict bits here: a changed sign of zero counts, NaN payloads do not matter
        assert new.tobytes() != w.tobytes(), (t, op, cnt)
        assert new[:1].tobytes() != w[:1].tobytes(), (t, op, cnt)
        assert not same_bits(C.model(t, w, o[1:], op)[0], new, bf16=bf), ("shift", t, op, cnt)
        if op in ("MIN", "MAX") and (bf or C.npdt(t).kind == "f"):
            assert not same_bits(C.model(t, o[:cnt], w, op)[0], new, bf16=bf), ("roles", t, op, cnt)
            if cnt >= 16:  # NaN in the window only, the origin only and both; both zero orders; a tie
                f = (w.astype(np.uint32) << 16).view(np.float32) if bf else w
                g = (o[:cnt].astype(np.uint32) << 16).view(np.float32) if bf else o[:cnt]
                assert (np.isnan(f) & ~np.isnan(g)).any() and (~np.isnan(f) & np.isnan(g)).any()
                assert (np.isnan(f) & np.isnan(g)).any()
                assert ((f == 0) & (g == 0) & (np.signbit(f) != np.signbit(g))).sum() >= 2
                assert ((f == g) & (f != 0)).any()
        if C.npdt(t).kind in "iu" and not bf:
            if op in ("SUM", "PROD") and cnt >= 16:
                wide = w.astype(object) + o[:cnt].astype(object) if op == "SUM" else w.astype(object) * o[:cnt].astype(object)
                info = np.iinfo(C.npdt(t))
                assert any(v > info.max or v < info.min for v in wide[:64]), (t, op)
            if op in ("LAND", "LOR", "LXOR") and cnt >= 16:
                assert (w == 0).any() and (o == 0).any() and (w > 1).any() and (o > 1).any()
        n += 1
    assert n > 400


def test_plan_sizes():
    """What the GPU test must see run (ran == planned) and fits a test's time."""
    full = C.plan(2, ["a", "c", "d"])
    assert C.ncases(full) == C.ncases(C.plan(3, ["a", "c", "d"]))
    by = {s: sum(len(ep["cases"]) for ep in full if ep["section"] == s) for s in "acd"}
    valid_pairs = sum(C.valid(op, t) for t in C.TYPES for op in C.OPS)
    assert valid_pairs == 8 * 12 + 3 * 9 + 2 * 4
    assert by["a"] == valid_pairs * 6 + len(C.SIZE_TYPES) * (8 + 4 + 1)
    assert by["c"] == (6 * 10 + 2) * 4 and by["d"] == 5
    assert C.ncases(C.plan(3, ["b"], C.SEAM_SCRATCH)) == 5 * 3 * 4 + 2
    # every window stays small enough to refill and compare every epoch
    for t in C.TYPES + ["uint8"]:
        assert C.window_elems(full, t) * C.esize(t) <= 40 << 20
