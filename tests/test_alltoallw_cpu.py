"""Alltoallw, the parts that need no GPU.

* tests/golden/alltoallw_golden.json (recorded from MPICH 3.3.2's
  MPI_Alltoallw by tests/golden/make_alltoallw_golden.sh) equals the numpy
  restatement of the type map (tests/spmd/alltoallw_cases.py `expected`) for
  every record at n = 2, 3, 4, so the fixture the device run is held to is
  pinned independently of the engine.
* The table reaches what it names: mixed unit widths in one launch, every
  empty-segment position, the deal past 4096 blocks, the run search; the
  geometry constants are the engine's.
* The ABI: mpigx_alltoallw is exported, declared in mpigx.h and has a
  prototype; the diagnostic entry point is declared in the diag header only; a
  NULL communicator is refused without a GPU.
* The new kernel's code object has no private segment.
* The mirror: the span check, and IN_PLACE with None send arguments.

On the parent commit the ABI, kernel and mirror tests fail: there is no
mpigx_alltoallw, no segw_pack_kernel and no Alltoallw_."""
import ctypes
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

import alltoallw_cases as AC  # noqa: E402
from test_kernel_resources_cpu import BUILD, LLVM, _kernel_private_sizes  # noqa: E402

CSRC = os.path.join(ROOT, "mpi.jl_amd", "csrc")


# --- the fixture -----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_model_reproduces_every_recorded_mpich_case(n):
    with open(os.path.join(HERE, "golden", "alltoallw_golden.json")) as f:
        gold = json.load(f)["runs"][str(n)]
    want = AC.expected(n)
    assert len(gold) == n
    for r in range(n):
        assert [g["case"] for g in gold[r]] == [w["case"] for w in want[r]]
        for g, w in zip(gold[r], want[r]):
            assert g == w, (n, r, g["case"])


# --- the table -------------------------------------------------------------------
def widths(s):
    """Unit widths of a packed side's blocks: pointer and packed prefixes 16-B aligned, as the engine has them."""
    out, at = [], 0
    for c, d, t in s["blocks"]:
        out.append(AC.unit_width(t, c, s["off"] + d, at))
        at += (c * AC.size_of(t) + 15) // 16 * 16
    return out


def test_geometry_constants_are_the_engines():
    common = open(os.path.join(CSRC, "common.hpp")).read()
    typed = open(os.path.join(CSRC, "typed.hpp")).read()
    assert int(re.search(r"constexpr int kThreads = (\d+);", common).group(1)) == AC.THREADS
    assert int(re.search(r"constexpr int kSegGrid = (\d+);", typed).group(1)) == AC.SEG_GRID
    header = open(os.path.join(ROOT, "include", "mpigx.h")).read()
    nmax = int(re.search(r"#define MPIGX_MAX_RANKS (\d+)", header).group(1))
    assert all(len(g["segs"]) <= nmax for g in AC.geometry())
    # the argument struct stays well under the 4 KiB kernel-argument limit: 64 B per segment
    fields = re.search(r"struct SegW \{(.*?)\};", typed, flags=re.S).group(1)
    per_seg = 0
    for decl in re.sub(r"//[^\n]*", "", fields).split(";"):
        decl = decl.strip()
        if decl:
            names = decl.count(",") + 1
            per_seg += names * (8 if "*" in decl or decl.startswith("long long") else 4)
    assert per_seg == 64 and nmax * per_seg + 128 < 2048


def test_table_reaches_what_it_names():
    ops = {o["name"]: o for o in AC.ops(3)}
    assert list(ops) == ["halo", "transpose", "mixed_widths", "plain", "empty_segments", "inplace"]
    # halo: a W = 8 column face, a contiguous row face, nothing to self, subarrays into the ghost cells
    for r in range(3):
        me = ops["halo"]["ranks"][r]
        assert me["send"]["blocks"][r][0] == 0 and me["recv"]["blocks"][r][0] == 0
        w = widths(me["send"])
        assert w[(r + 1) % 3] == 8 and AC.contiguous(me["send"]["blocks"][(r - 1) % 3][2])
        assert all(t[0] == "subarray" for c, _, t in me["recv"]["blocks"] if c)
    # transpose: a different subarray per peer, ragged, received contiguously at odd displacements
    t0 = ops["transpose"]["ranks"][0]
    assert len({repr(t) for _, _, t in t0["send"]["blocks"]}) == 3
    assert len({c * AC.size_of(t) for c, _, t in t0["recv"]["blocks"]}) > 1
    assert all(d % 2 == 1 and AC.contiguous(t) for _, d, t in t0["recv"]["blocks"])
    assert AC.packs(ops["transpose"], 0) == (True, False)
    # mixed widths in one launch: 16, 4 and 1, the W = 16 block with several instances
    for r in range(3):
        s = ops["mixed_widths"]["ranks"][r]["send"]
        assert sorted(widths(s)) == [1, 4, 16]
        c, d, t = s["blocks"][r]
        assert widths(s)[r] == 16 and c > 1 and d % 16 == 0
        assert len(AC.runs_of(AC.HOLES)) == 2 and widths(s)[(r + 2) % 3] == 1
        c, d, t = s["blocks"][(r + 1) % 3]
        assert t == AC.I4 and d % 8 == 4
    # no pack launch on either side
    assert all(AC.packs(ops["plain"], r) == (False, False) for r in range(3))
    assert any(d % 2 for r in range(3) for _, d, _ in ops["plain"]["ranks"][r]["send"]["blocks"])
    # every empty-segment position on a side that is packed
    seen = set()
    for n in (3, 4):
        op = AC.empties(n)
        for r in range(n):
            for which, packed in zip(("send", "recv"), AC.packs(op, r)):
                cs = [c for c, _, _ in op["ranks"][r][which]["blocks"]]
                if not any(cs):
                    seen.add(f"all_zero_{which}")
                if not packed:
                    continue
                nz = [i for i, c in enumerate(cs) if c]
                if cs[0] == 0:
                    seen.add("first")
                if cs[-1] == 0:
                    seen.add("last")
                if any(c == 0 for c in cs[nz[0]:nz[-1]]):
                    seen.add("between")
        if n == 3:
            assert seen == {"first", "last", "between", "all_zero_send", "all_zero_recv"}, seen
    # IN_PLACE: a different derived type per peer, none contiguous, both ends of a block equally long
    ip = ops["inplace"]
    for r in range(3):
        blocks = ip["ranks"][r]["recv"]["blocks"]
        assert ip["ranks"][r]["send"] is None and len({repr(t) for _, _, t in blocks}) == 3
        assert not any(AC.contiguous(t) for _, _, t in blocks)
        for q in range(3):
            c, _, t = blocks[q]
            c2, _, t2 = ip["ranks"][q]["recv"]["blocks"][r]
            assert c * AC.size_of(t) == c2 * AC.size_of(t2) > 0
    # every allocation has slack on both sides of its blocks and a position-dependent prefill
    for op in ops.values():
        for me in op["ranks"]:
            for s in (me["send"], me["recv"]):
                if s is None:
                    continue
                used = [AC.span(t, c, s["off"] + d) for c, d, t in s["blocks"] if c] or [(AC.SLACK, AC.SLACK)]
                assert min(lo for lo, _ in used) >= AC.SLACK and max(hi for _, hi in used) <= len(s["buf"]) - AC.SLACK
                assert len(set(s["buf"][:AC.SLACK].tolist())) > 8


def test_geometry_cases_reach_the_launch_arithmetic():
    G = {g["name"]: g for g in AC.geometry()}

    def units(g):
        return [c * AC.size_of(t) // max(1, w) for (t, c, _, _), w in zip(g["segs"], g["want_w"])]

    T = AC.THREADS
    assert units(G["unit_counts"]) == [0, 1, T - 1, T, T + 1, 2 * T + 1]
    g = AC.deal(units(G["unit_counts"]), G["unit_counts"]["want_w"])
    # none for the empty segment, one for the 1-unit one; 257 units on one block: a second stride for thread 0
    assert g == [0, 1, 1, 1, 1, 3]
    assert all(0 < b <= -(-u // T) for b, u in zip(g[1:], units(G["unit_counts"])[1:]))
    # past the deal: more units than 4096 blocks x 256 threads; the small segment keeps its one block
    big = G["past_the_grid"]
    u = units(big)
    assert sum(u) > AC.SEG_GRID * T and u[0] == 3 and u[1] * 2 < (3 << 20)
    g = AC.deal(u, big["want_w"])
    assert g[0] == 1 and AC.SEG_GRID - 1 <= g[1] <= AC.SEG_GRID and -(-u[1] // T) > g[1]
    share = -(-u[1] // g[1])
    assert share > T and u[1] % share != 0  # a second stride per thread, and a short last block
    # equal byte lengths, widths 16 and 1: the deal goes by bytes, not units
    both = G["w16_beside_w1"]
    lens = [c * AC.size_of(t) for t, c, _, _ in both["segs"]]
    assert lens[0] == lens[1] and both["want_w"] == [16, 1]
    assert units(both) == [lens[0] // 16, lens[0]] and AC.deal(units(both), [16, 1]) == [1, 1]
    # three runs of unequal length; 7-byte instances straddle the share boundaries
    three = G["three_runs_straddle"]
    t, c, _, _ = three["segs"][0]
    assert AC.runs_of(t) == [(0, 1), (2, 2), (8, 4)] and AC.size_of(t) == 7  # no two adjacent, no two equally long
    g = AC.deal(units(three), [1])[0]
    share = -(-units(three)[0] // g)
    assert g > 1 and share % 7 != 0
    # the typed address alone lowers W
    low = G["typed_base_lowers_w"]
    assert len({repr(t) for t, _, _, _ in low["segs"]}) == 1 and all(o % 16 == 0 for _, _, _, o in low["segs"])
    assert [AC.unit_width(t, c, AC.SLACK + d, o) for t, c, d, o in low["segs"]] == [16, 8, 4, 2, 1] == low["want_w"]
    odd = G["odd_pointer"]
    assert odd["base"] % 2 == 1 and odd["want_w"] == [1, 1]
    for g in G.values():  # no two segments overlap, typed or packed
        tb, off, pb = AC.geometry_buffers(g)
        seen_t, seen_p = np.zeros(tb, bool), np.zeros(pb, bool)
        for t, c, d, o in g["segs"]:
            a = AC.addrs(t, c, off + d)
            assert not seen_t[a].any() and not seen_p[o:o + len(a)].any()
            seen_t[a] = True
            seen_p[o:o + len(a)] = True
        assert g["want_w"] == [AC.unit_width(t, c, off + d, o) for t, c, d, o in g["segs"]]


# --- the ABI -----------------------------------------------------------------------
def test_alltoallw_is_exported_declared_and_prototyped():
    import mpigx
    from mpigx._lib import PROTOTYPES

    assert hasattr(mpigx.lib(), "mpigx_alltoallw") and "mpigx_alltoallw" in PROTOTYPES
    public = re.sub(r"/\*.*?\*/", "", open(mpigx.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"^int mpigx_alltoallw\(", public, flags=re.M)
    assert len(PROTOTYPES["mpigx_alltoallw"][1]) == 9


def test_diagnostic_entry_point_is_declared_in_the_diag_header_only():
    import mpigx
    from mpigx._lib import PROTOTYPES

    assert "mpigx_pack_segments_w" in PROTOTYPES and hasattr(mpigx.lib(), "mpigx_pack_segments_w")
    assert "mpigx_pack_segments_w" in open(mpigx.DIAG_HEADER_PATH).read()
    assert "mpigx_pack_segments_w" not in open(mpigx.HEADER_PATH).read()


def test_null_communicator_is_refused_without_a_gpu():
    import mpigx
    from mpigx import consts as K

    one = (ctypes.c_int * 1)(0)
    assert mpigx.lib().mpigx_alltoallw(None, one, one, one, None, one, one, one, None) == K.MPI_ERR_COMM


# --- the built kernel ----------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(BUILD, "copy.o")) or
                    not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="kernel objects not built (run __graft_entry__.build())")
def test_segw_pack_kernel_has_no_private_segment(tmp_path):
    sizes = _kernel_private_sizes(os.path.join(BUILD, "copy.o"), str(tmp_path))
    mine = {k: v for k, v in sizes.items() if "segw_pack_kernel" in k}
    assert mine, sorted(sizes)
    assert all(v == 0 for v in mine.values()), mine


# --- the mirror ------------------------------------------------------------------------
class FakeLibmpi:
    def __init__(self):
        self.calls = []

    def MPI_Alltoallw(self, *a):
        self.calls.append(a)
        return 0


def fake_comm(api, n):
    return api.Comm(None, 0, n, None, host=0x44000000)


def test_mirror_span_check_raises(monkeypatch):
    import mpigx as MPI
    from mpigx import api

    fake = FakeLibmpi()
    monkeypatch.setattr(api.hostmpi, "lib", lambda: fake)
    comm = fake_comm(api, 2)
    f8 = np.dtype("f8")
    send, recv = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    ok = ([1, 2], [0, 16], [f8, f8])
    MPI.Alltoallw_(send, *ok, recv, [2, 4], [0, 32], [f8, f8], comm)
    assert len(fake.calls) == 1
    with pytest.raises(AssertionError):  # the last receive block ends at byte 72
        MPI.Alltoallw_(send, *ok, recv, [2, 5], [0, 32], [f8, f8], comm)
    with pytest.raises(AssertionError):  # a send block before the buffer
        MPI.Alltoallw_(send, [1, 2], [-8, 16], [f8, f8], recv, [2, 4], [0, 32], [f8, f8], comm)
    # the TRUE upper bound counts: a resized type whose extent is below its span
    T = MPI.Types
    col = T.commit_(T.create_resized(T.create_vector(4, 1, 4, MPI.Datatype(f8)), 0, 8))  # spans 104 bytes
    with pytest.raises(AssertionError):
        MPI.Alltoallw_(send, *ok, recv, [1, 0], [0, 0], [col, f8], comm)
    # an empty block may point anywhere
    MPI.Alltoallw_(send, *ok, recv, [0, 8], [4096, 0], [col, f8], comm)
    assert len(fake.calls) == 2


def test_mirror_accepts_in_place_with_none_send_arguments(monkeypatch):
    import mpigx as MPI
    from mpigx import api

    fake = FakeLibmpi()
    monkeypatch.setattr(api.hostmpi, "lib", lambda: fake)
    buf = np.zeros(64, np.uint8)
    i4 = MPI.Datatype(np.dtype("i4"))
    MPI.Alltoallw_(MPI.IN_PLACE, None, None, None, buf, [2, 3], [0, 8], [i4, np.dtype("f4")], fake_comm(api, 2))
    (a,) = fake.calls
    assert a[0].value == api._IN_PLACE_PTR.value and a[1:4] == (None, None, None)
    assert a[4].value == buf.ctypes.data and list(a[5]) == [2, 3] and list(a[6]) == [0, 8]
    assert list(a[7]) == [i4.host, MPI.Datatype(np.dtype("f4")).host] and a[8] == 0x44000000
