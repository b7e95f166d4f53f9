"""RMA data paths past 12 elements (tests/spmd/rma_data_worker.py, plan and
model in tests/spmd/rma_data_cases.py): Accumulate / Get_accumulate for every
valid (op, type) of the 13 accumulate types — bf16 included, against the bf16
oracle definition, parity unpinned — at counts that reach the main loop, the
tail and the block cap of acc_kernel; Get_accumulate and Fetch_and_op across
the scratch-slot chunk seams; Put / Get of byte ranges through every
block_copy branch, head, slice rounding and the block cap; 40 non-commuting
accumulates per target without a flush (the 16-slot envelope ring wraps
twice) and multi-origin accumulates into one range.  Every window and result
allocation is compared whole, guards included, bit for bit against the
MPICH-pinned model.  tests/test_rma_data_cpu.py checks that the plan reaches
the regions it names."""
import json
import os
import sys

import pytest

from spmd_launch import ROOT, launch
from test_rma_gpu import ENV

sys.path.insert(0, os.path.join(ROOT, "tests", "spmd"))
import rma_data_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

XDEV = dict(ENV, MPIGX_PEER_MEM="xdev", MPIGX_SHARED_GATE="0")  # as tests/test_fuzz_gpu.py


def run(n, sections, env, scratch=None):
    env = dict(env, RMA_DATA_SECTIONS=",".join(sections))
    if scratch:
        env["MPIGX_RMA_SCRATCH"] = str(scratch)
    rcs, outs = launch(os.path.join(ROOT, "tests", "spmd", "rma_data_worker.py"), n, timeout=120, extra_env=env)
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}" for r, (rc, o) in enumerate(zip(rcs, outs)))
    res = [json.loads(l) for o in outs for l in o.splitlines() if l.startswith("{") and '"nfail"' in l]
    assert len(res) == n, msg
    planned = C.ncases(C.plan(n, sections, scratch or C.DEFAULT_SCRATCH))
    print(json.dumps({"n": n, "sections": sections, "planned": planned, "ran": [x["ran"] for x in res],
                      "nfail": [x["nfail"] for x in res], "per": res[0]["per"],
                      "seconds": [x["seconds"] for x in res]}), flush=True)  # shown with -s
    for x in res:
        assert x["nfail"] == 0, (x["first_failures"], x["failed"])
        assert x["ran"] == planned, (x["ran"], planned)  # nothing silently skipped
    assert all(rc == 0 for rc in rcs), msg
    return res


@pytest.mark.parametrize("n", [2, 3])
def test_rma_data_paths(n):
    """(~14 s) a, c, d: the (op, type) matrix at 1024 / 1025 / 4099 elements and the capped counts, Put / Get byte sizes x alignments under fence and lock, 40 unflushed non-commuting accumulates and multi-origin accumulates; whole windows and result allocations against the model."""
    run(n, ["a", "c", "d"], ENV)


@pytest.mark.parametrize("n", [2, 3])
def test_rma_chunk_seams(n):
    """(~7 s) b: MPIGX_RMA_SCRATCH=4096 (slot 2048 / 1280 bytes): Get_accumulate SUM / REPLACE / NO_OP at per - 1, per, per + 1 and 3 per + 7 elements for one type of each element size, Fetch_and_op on bf16 and complex128."""
    res = run(n, ["b"], ENV, scratch=C.SEAM_SCRATCH)
    slot = {2: 2048, 3: 1280}[n]
    for x in res:
        assert x["per"] == {t: slot // C.esize(t) for t in C.SIZE_TYPES}


def test_rma_data_paths_cross_gpu_protocol():
    """(~4 s) e: n = 3 with MPIGX_PEER_MEM=xdev and no host gate (the coherent-pull fences of the production signalling): the 4099-count matrix row, the chunk seams and one Put / Get alignment sweep."""
    run(3, ["a4099", "b", "c1"], XDEV, scratch=C.SEAM_SCRATCH)
