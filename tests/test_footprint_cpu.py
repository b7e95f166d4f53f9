"""The footprint harness (tests/footprint.py) can fail, and its case table
covers what it claims: verifier mutation checks on numpy arrays, coverage
conditions on cases(n), and every case's expected value computed through the
models without a GPU (a case the model cannot express fails here, before it
reaches the GPU box)."""
import numpy as np
import pytest

import footprint as F
from oracle import mpich_model as M

NS = (3, 5, 7, 8)


def _buf(readonly=False, off=12):
    x = np.arange(37, dtype=np.float32) * 1.5
    return F.Guarded(x, off, rank=2, salt=9, readonly=readonly, expect=None if readonly else x, npdt=np.float32)


def _flip(g, at):
    got = g.image.copy()
    got[at] ^= 0x40
    return got


def test_untouched_buffer_is_clean():
    for ro in (False, True):
        g = _buf(ro)
        assert F.verify(g, g.image.copy()) == []


@pytest.mark.parametrize("where", ["pre_last", "post_first", "post_last", "pad"])
def test_one_flipped_guard_byte_is_reported_with_its_location(where):
    g = _buf()
    assert g.lo == F.PRE + 12 and g.hi == g.lo + 37 * 4 and g.image.size == g.hi + F.POST
    at, kind = {"pre_last": (F.PRE - 1, "pre"), "post_first": (g.hi, "post"), "post_last": (g.image.size - 1, "post"),
                "pad": (F.PRE + 5, "pad")}[where]
    found = F.verify(g, _flip(g, at))
    assert [(f["kind"], f["offset"]) for f in found] == [(kind, at)], found
    assert found[0]["nbad"] == 1


def test_read_only_buffer_reports_any_changed_byte():
    g = _buf(readonly=True)
    for at, region in ((0, "pre"), (F.PRE + 3, "pad"), (g.lo + 17, "payload"), (g.hi - 1, "payload"), (g.hi, "post"),
                       (g.image.size - 1, "post")):
        found = F.verify(g, _flip(g, at))
        assert [(f["kind"], f["offset"], f["region"]) for f in found] == [("readonly", at, region)], found


def test_payload_difference_is_reported_and_nan_matches_nan():
    g = _buf()
    found = F.verify(g, _flip(g, g.lo + 4 * 5 + 1))
    assert [(f["kind"], f["first_bad_elem"]) for f in found] == [("payload", 5)], found
    x = np.array([1.0, np.nan, 3.0], np.float32)
    g = F.Guarded(x, 4, 0, 1, expect=x, npdt=np.float32)
    got = g.image.copy()
    got[g.lo + 4: g.lo + 8] = np.array([0xFFC00001], np.uint32).view(np.uint8)  # another NaN
    assert F.verify(g, got) == []


def test_pattern_depends_on_position_rank_and_salt():
    a = F.pattern(4096, 0, 0)
    assert len(set(a[:256].tolist())) == 256  # 131 is odd: every byte value within 256 positions
    assert not np.array_equal(a, F.pattern(4096, 1, 0)) and not np.array_equal(a, F.pattern(4096, 0, 1))
    assert not np.array_equal(a[:-16], a[16:])  # a guard copied 16 B further differs


@pytest.mark.parametrize("align", [1, 2, 4, 8])
def test_offset_table_mixes_alignment_across_ranks(align):
    for n in NS:
        so = [F.send_off(r, align, align) for r in range(n)]
        ro = [F.recv_off(r, align, align) for r in range(n)]
        assert all(o % align == 0 and 0 <= o < F.ALIGN for o in so + ro)
        assert any(s % 16 == 0 and q % 16 == 0 for s, q in zip(so, ro)), "a rank aligned on both"
        assert any(s % 16 != 0 and q % 16 == 0 for s, q in zip(so, ro)), "a rank misaligned on send only"
        assert any(s % 16 == 0 and q % 16 != 0 for s, q in zip(so, ro)), "a rank misaligned on recv only"
        assert len({q % 16 for q in ro}) >= 2
        if align < 4:  # both block_copy branches and the byte fallback for 1- and 2-byte types
            assert len({q % 4 for q in ro}) >= 2
            pairs = {(d ^ s) for d in ro for s in so}
            assert any(p % 16 == 0 for p in pairs) and any(p % 16 and p % 4 == 0 for p in pairs) \
                and any(p % 4 for p in pairs)


def _required_pairs():
    req = {("allreduce", a) for a, _ in F.AR_ALGOS} | {("allreduce", p) for p in ("ring1", "ring2", "pullpush_slices3",
                                                                                   "linear")}
    req |= {("reduce", p) for p in ("oneshot", "twoshot", "ll", "zc")}
    req |= {("bcast", f"{m}_{s}") for m in ("direct", "sag", "relay") for s in ("staged", "zc")}
    req |= {(c, p) for c in ("allgather", "alltoall", "reduce_scatter_block", "reduce_scatter") for p in ("staged", "zc")}
    req |= {(c, p) for c in ("scan", "exscan") for p in ("pp", "pull", "staged")}
    return req


@pytest.mark.parametrize("n", NS)
def test_case_table_coverage(n):
    cs = F.cases(n)
    assert cs == F.cases(n), "deterministic"
    assert len({c["id"] for c in cs}) == len(cs)
    have = {(c["coll"], c["path"]) for c in cs}
    assert _required_pairs() <= have, _required_pairs() - have
    # the fuzz worker's algorithm names, all of them
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "spmd", "fuzz_worker.py")).read()
    algos = next(ast.literal_eval(s.value) for s in ast.parse(src).body
                 if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", "") == "ALGOS")
    names = {c["knobs"].get("ALGO") for c in cs if c["coll"] == "allreduce"}
    assert set(algos) <= names, set(algos) - names
    # every dtype with every family
    dts = {d for d, _ in F.DTYPE_OPS}
    assert {"INT8_T", "FLOAT", "DOUBLE", "C_DOUBLE_COMPLEX"} <= dts and dts & {"INT16_T", "BFLOAT16"}
    for fam in ("reducing", "moving", "scan"):
        assert {c["dtype"] for c in cs if F.FAMILY[c["coll"]] == fam} == dts, fam
    # every count shape of every dtype, and an op of each kind where roles matter
    for d in dts:
        assert {c["count"] for c in cs if c["dtype"] == d} >= set(F.counts_for(d, n)), d
    assert {c["op"] for c in cs} >= {"SUM", "MIN", "MAX", "PROD"}
    ragged = sum((c["count"] * F.esize(c["dtype"])) % 16 != 0 for c in cs)
    assert 2 * ragged >= len(cs), (ragged, len(cs))
    # ring: integer types only; both roots of Reduce on every path; IN_PLACE where the call has it
    assert all(c["dtype"] in F.INT_TYPES for c in cs if c["path"].startswith("ring"))
    for p in ("oneshot", "twoshot", "ll", "zc"):
        assert {c["root"] for c in cs if (c["coll"], c["path"]) == ("reduce", p)} == {0, n - 1}
    for coll in ("allreduce", "allgather", "alltoall", "scan", "exscan", "reduce_scatter_block", "reduce_scatter"):
        for zc in (0, 1):
            if coll == "alltoall" and zc:
                continue  # the zero-copy Alltoall is out of place only (gather_like)
            assert {c["inplace"] for c in cs if c["coll"] == coll and c["knobs"].get("ZC", 0) == zc} == {False, True}, coll
    assert any(0 in c["counts"] for c in cs if c["coll"] == "reduce_scatter")
    # the forced LL paths apply at every size of the table (else they would silently run staged)
    assert all(F.ll_ok(c, n) for c in cs)
    assert any(not F.ll_ok(dict(c, count=1 << 20), n) for c in cs if c["knobs"].get("ALGO") == "ll")


def test_small_arena_and_complex_tables():
    cs = F.small_arena_cases(3)
    assert {c["coll"] for c in cs} == {"allreduce", "reduce", "bcast", "reduce_scatter_block", "reduce_scatter"}
    assert ("allreduce", "twoshot") in {(c["coll"], c["path"]) for c in cs}
    assert all(F.rounds(c, 3) >= 3 for c in cs), [F.rounds(c, 3) for c in cs]
    assert all(c["knobs"]["ZC"] == 0 for c in cs)
    cx = F.complex_cases(3)
    assert {(c["dtype"], c["path"]) for c in cx} == {(d, p) for d in ("C_DOUBLE_COMPLEX", "C_FLOAT_COMPLEX")
                                                     for p in ("twoshot", "pull")}
    assert F.comp_align("C_DOUBLE_COMPLEX") == 8 and F.comp_align("C_FLOAT_COMPLEX") == 4
    offs = {F.recv_off(r, 16, 8) for r in range(3)} | {F.send_off(r, 16, 8) for r in range(3)}
    assert 8 in offs


@pytest.mark.parametrize("n,table", [(3, "main"), (5, "main"), (8, "main"), (3, "small"), (3, "complex")])
def test_expected_values_and_buffers_without_a_gpu(n, table):
    cs = {"main": F.cases, "small": F.small_arena_cases, "complex": F.complex_cases}[table](n)
    for c in cs:
        ins = F.inputs(c, n)
        assert len(ins) == n and all(x.size == F.send_elems(c, n) for x in ins)
        outs = F.expected(c, n, ins)
        assert len(outs) == n
        npdt = np.dtype(M.DTYPES[c["dtype"]][1])
        for r in range(n):
            none_ok = (c["coll"] == "reduce" and r != c["root"]) or (c["coll"] == "exscan" and r == 0)
            assert (outs[r] is None) == none_ok, (c, r)
            if outs[r] is not None:
                assert outs[r].dtype == npdt and outs[r].shape == (F.recv_elems(c, n, r),), (c, r)
            sg, rg = F.buffers(c, n, r, ins, outs)
            assert (sg is None) == (c["coll"] == "bcast" or (c["inplace"] and not (c["coll"] == "reduce" and r != c["root"])))
            assert rg is not None and (sg is None or sg.readonly)
            # an untouched out-of-place recvbuf must not pass as a result
            if rg.expect is not None and rg.nbytes and not c["inplace"]:
                assert any(f["kind"] == "payload" for f in F.verify(rg, rg.image))
            a = F.comp_align(c["dtype"])
            assert (rg.lo - F.PRE) == F.recv_off(r, npdt.itemsize, a)
