"""Derived datatypes in Gatherv / Scatterv / Allgatherv / Alltoallv and in
one-sided Get / Put on device buffers.

* tests/spmd/strided_worker.py on ROCm tensors must reproduce, byte for byte,
  the records MPICH 3.3.2 produced on host arrays
  (tests/golden/strided_golden.json): struct arrays through MPI.jl's
  signatures, matrix columns through a resized vector type, vector <->
  contiguous Alltoallv, subarray and IN_PLACE Allgatherv, typed Put / Get
  (vector, halo face, 3-D subarray, struct, unequal counts, dynamic window,
  PROC_NULL, ordered overlapping Puts), plus the engine's own error classes.
  n = 3 is in the default selection, n = 2 and 4 are marked slow.
* The index arithmetic of the two kernels (copy.hip seg_pack_kernel,
  typed_xfer_kernel) against the numpy restatement of the type map
  (tests/spmd/strided_cases.py), at sizes taken from their launch geometry:
  256 threads per block, 4096 blocks dealt per launch.

On the parent commit every case fails with MPI_ERR_TYPE (class 3): the
v-collectives refused non-contiguous types and Get / Put every derived one."""
import json
import os
import sys

import pytest

from spmd_launch import ROOT, launch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "spmd"))

ENV = {"MPIGX_DEVICE": "0", "MPIGX_INIT_TIMEOUT_MS": "60000", "MPIGX_MAX_BLOCKS": "16", "MPIGX_TIMEOUT_MS": "30000",
       "MPIGX_STAGING_BYTES": str(32 << 20), "MPIGX_TEST_ARRAYTYPE": "ROCArray"}
DEV_CHECKS = ["Put_size_mismatch", "Get_size_mismatch", "Put_run_capacity", "Put_past_window", "Get_past_window",
              "refused_calls_wrote_nothing", "Put_64_runs"]


def run_worker(n, tmp_path):
    env = dict(ENV, DT_OUT=str(tmp_path / "st"))
    rcs, outs = launch(os.path.join(ROOT, "tests", "spmd", "strided_worker.py"), n, timeout=600, extra_env=env)
    recs = {}
    for r in range(n):
        p = tmp_path / f"st.{r}"
        if p.exists():
            recs[r] = json.loads(p.read_text())
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}\n{recs.get(r, {}).get('failed')}"
                    for r, (rc, o) in enumerate(zip(rcs, outs)))
    assert all(rc == 0 for rc in rcs), msg
    with open(os.path.join(ROOT, "tests", "golden", "strided_golden.json")) as f:
        gold = json.load(f)["runs"][str(n)]
    for r in range(n):
        assert recs[r]["device"] is True and recs[r]["failed"] is None
        assert [c["check"] for c in recs[r]["dev_checks"]] == DEV_CHECKS
        for c in recs[r]["dev_checks"]:
            assert c["got"] == c["want"], (r, c["check"], c["got"], c["want"])
        assert len(recs[r]["records"]) == len(gold[r])
        for got, want in zip(recs[r]["records"], gold[r]):
            assert got == want, (r, got["case"], got, want)


def test_strided_scenarios_device_match_mpich_n3(tmp_path):
    """(~4 s) Typed v-collectives and Get / Put reproduce MPICH's records at n = 3 (one launch)."""
    run_worker(3, tmp_path)


@pytest.mark.slow
@pytest.mark.parametrize("n", [2, 4])
def test_strided_scenarios_device_match_mpich(n, tmp_path):
    """(~9 s) The same at n = 2 and 4."""
    run_worker(n, tmp_path)


def test_kernel_index_arithmetic(tmp_path):
    """(~3 s) seg_pack_kernel and typed_xfer_kernel against the numpy type map for W = 1, 2, 4, 8, 16 (one process)."""
    env = dict(ENV, DT_OUT=str(tmp_path / "ix"))
    rcs, outs = launch(os.path.join(ROOT, "tests", "spmd", "strided_index_worker.py"), 1, timeout=600, extra_env=env)
    p = tmp_path / "ix.0"
    rec = json.loads(p.read_text()) if p.exists() else {}
    assert rcs == [0] and rec.get("failed") is None, f"{outs[0][-3000:]}\n{rec.get('failed')}"
    # 5 widths x (2 layouts x pack + unpack, 3 shapes x Get + Put) + the two past the 4096-block deal
    assert rec["cases"] == 5 * (4 + 6) + 2 + 2
