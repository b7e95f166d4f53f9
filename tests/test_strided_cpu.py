"""Derived datatypes in the v-collectives and in Get / Put: what can be
checked without a GPU.

* tests/golden/strided_golden.json (recorded from MPICH 3.3.2 by
  tests/golden/make_strided_golden.sh) equals the numpy restatement of MPI's
  type map (tests/spmd/strided_cases.py `expected`) for every record, so the
  fixture the device run is held to is pinned independently of the engine.
* The Python mirror's operand plumbing: an MPI.Buffer gives each side of a
  v-collective and of Get / Put its own (count, datatype handle); a structured
  numpy dtype becomes a struct datatype; plain arrays keep their predefined
  types.
* The new diagnostic entry point is declared in the header and in PROTOTYPES."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "spmd"))
sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))

import strided_cases as SC  # noqa: E402


@pytest.mark.parametrize("n", [2, 3, 4])
def test_fixture_equals_the_numpy_type_map(n):
    with open(os.path.join(HERE, "golden", "strided_golden.json")) as f:
        gold = json.load(f)["runs"][str(n)]
    want = SC.expected(n)
    assert len(gold) == n
    for r in range(n):
        assert [g["case"] for g in gold[r]] == [w["case"] for w in want[r]]
        for g, w in zip(gold[r], want[r]):
            assert g == w, (n, r, g["case"])


def test_scenarios_cover_what_they_claim():
    """The cases the fixture is meant to hold are really in it."""
    ops = {o["name"]: o for o in SC.ops(3)}
    for nm in ("boundary", "ntuple3"):
        for k in ("gatherv", "scatterv", "allgatherv", "alltoallv"):
            assert f"{k}_{nm}" in ops
    assert 0 in ops["gatherv_boundary"]["counts"] and len(set(ops["gatherv_boundary"]["counts"])) > 1
    assert SC.size_of(SC.BOUNDARY) == 11 and SC.typemap(SC.BOUNDARY)[2] == 24
    cols = ops["columns_scatterv_f64"]
    assert len(set(cols["counts"])) > 1 and sum(cols["counts"]) == 7
    spec = cols["ranks"][0]["send"]["spec"]
    assert SC.typemap(spec)[2] == 8 < SC.span(spec, 1)[1]  # extent below the true extent: instances interleave
    assert ops["columns_scatterv_c128_off8"]["ranks"][0]["send"]["off"] == 8
    rma = ops["rma"]
    assert any(x["dyn"] for x in rma["puts"]) and any(x["target"] < 0 for x in rma["puts"])
    assert any(x["ocount"] != x["tcount"] for x in rma["puts"])
    # untouched bytes are part of every record: buffers start as 0xEE and keep it where no type map reaches
    rec = SC.expected(3)[2][0]
    assert "ee" in rec["recv"]


def test_type_map_restatement():
    i4 = np.dtype("i4")
    o, lb, ext = SC.typemap(("vector", 3, 2, 4, i4))
    assert o.tolist() == [*range(0, 8), *range(16, 24), *range(32, 40)] and (lb, ext) == (0, 40)
    o, lb, ext = SC.typemap(("subarray", (4, 6), (2, 3), (1, 2), i4))
    assert o[::4].tolist() == [32, 36, 40, 56, 60, 64] and ext == 96
    o, lb, ext = SC.typemap(("resized", ("vector", 5, 1, 7, np.dtype("f8")), 0, 8))
    assert o[::8].tolist() == [0, 56, 112, 168, 224] and ext == 8
    buf = SC.data(64, 0)
    out = SC.blank(64)
    SC.unpack(out, SC.pack(buf, SC.BOUNDARY, 2), SC.BOUNDARY, 2)
    keep = SC.addrs(SC.BOUNDARY, 2)
    assert np.array_equal(out[keep], buf[keep]) and (np.delete(out, keep) == SC.FILL).all()


def test_mirror_operand_plumbing():
    import mpigx as MPI
    from mpigx import api, rma

    class FakeType:
        val, host = 0x3D000123, 0x8C000005

    arr = np.zeros(48, np.uint8)
    b = MPI.Buffer(arr, 2, MPI.Datatype(FakeType.val, "fake", FakeType.host))
    # v-collectives: each side takes its own datatype
    assert api._vtype(b, MPI.Datatype(np.float64)) == FakeType.val
    assert api._vtype(arr, MPI.Datatype(np.float64)) == MPI.Datatype(np.float64).val
    assert api._vtype(None, MPI.Datatype(np.int16)) == MPI.Datatype(np.int16).val
    # Get / Put: (count, engine handle, host handle)
    assert rma._operand(b) == (2, FakeType.val, FakeType.host)
    f = np.zeros(5, np.float32)
    assert rma._operand(f) == (5, MPI.Datatype(np.float32).val, MPI.Datatype(np.float32).val)
    assert rma._operand(f, 3)[0] == 3
    (oc, odt, _), (tc, tdt, _), t, disp, win = rma._xfer_args(f, (1, "w"), None)
    assert (oc, odt, tc, tdt, t, disp, win) == (5, odt, 5, odt, 1, 0, "w")
    (oc, odt, _), (tc, tdt, th), t, disp, win = rma._xfer_args(f, (4, 1, 16, "w"), (2, b.datatype))
    assert (oc, tc, tdt, th, t, disp) == (4, 2, FakeType.val, FakeType.host, 1, 16)


def test_structured_dtype_becomes_a_struct_type():
    import mpigx as MPI

    dt = MPI.Datatype(SC.BOUNDARY)
    assert (dt.val & 0xFF000000) == 0x3D000000  # a derived handle of the engine, not a predefined type
    assert MPI.Types.size(dt) == 11 and MPI.Types.extent(dt) == (0, 24)
    b = MPI.Buffer(np.zeros(72, np.uint8), 3, dt)
    assert (b.count, b.datatype.val) == (3, dt.val)


def test_pack_segments_is_declared():
    import mpigx
    from mpigx._lib import PROTOTYPES

    assert "mpigx_pack_segments" in PROTOTYPES
    assert "mpigx_pack_segments" in open(mpigx.DIAG_HEADER_PATH).read()
    assert "mpigx_pack_segments" not in open(mpigx.HEADER_PATH).read()
