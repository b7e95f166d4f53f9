"""Accumulate / Get_accumulate through non-contiguous derived datatypes on
device windows (acc_typed_kernel; tests/spmd/acc_typed_worker.py, table and
model in tests/spmd/acc_typed_cases.py): every element size, SUM / MAX / BXOR
/ REPLACE / NO_OP, vectors, hvectors, subarrays, interleaved resized vectors,
structs with holes, a 64-run target, a dynamic window, every loop region of
the kernel, the Get_accumulate chunk seams inside runs and instances,
unflushed overlapping posts and a three-origin sum.  Whole windows, result and
origin allocations must equal the recorded MPICH run bit for bit
(tests/golden/acc_typed_golden.json) and the model (bf16: the model only);
each refusal must return its error class and leave the window untouched.
tests/test_acc_typed_cpu.py checks that the table reaches what it names."""
import json
import os
import sys

import pytest

from spmd_launch import ROOT, launch
from test_rma_gpu import ENV

sys.path.insert(0, os.path.join(ROOT, "tests", "spmd"))
import acc_typed_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def test_acc_typed_matches_mpich_and_model():
    """(~4 s) n = 3, MPIGX_RMA_SCRATCH=4096 (1280-byte slots): the whole table of acc_typed_cases.py against the MPICH fixture and the model, and the six refusals."""
    env = dict(ENV, MPIGX_RMA_SCRATCH=str(C.SCRATCH))
    rcs, outs = launch(os.path.join(ROOT, "tests", "spmd", "acc_typed_worker.py"), C.N, timeout=120, extra_env=env)
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}" for r, (rc, o) in enumerate(zip(rcs, outs)))
    res = [json.loads(l) for o in outs for l in o.splitlines() if l.startswith("{") and '"nfail"' in l]
    assert len(res) == C.N, msg
    res.sort(key=lambda x: x["rank"])
    print(json.dumps({"seconds": [x["seconds"] for x in res], "nfail": [x["nfail"] for x in res]}), flush=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "acc_typed_golden.json")))["records"]
    for x, gold in zip(res, golden):
        assert x["failed"] is None and x["device"], x["failed"]
        assert [r["case"] for r in x["records"]] == [c["id"] for c in C.CASES]  # nothing skipped
        assert x["nfail"] == 0, x["first_failures"]  # the model, whole allocations (worker)
        mine = {r["case"]: r for r in x["records"]}
        for g in gold:  # the fixture, exactly
            assert mine[g["case"]] == g, (x["rank"], g["case"])
        assert [(r["case"], r["rc"], r["untouched"]) for r in x["refused"]] == [(r["id"], r["want"], True)
                                                                               for r in C.REFUSALS]
    assert all(rc == 0 for rc in rcs), msg
