"""Alltoallw on device buffers: one datatype and one byte displacement per peer.

* tests/spmd/alltoallw_worker.py on ROCm tensors must reproduce, byte for
  byte, the records MPICH 3.3.2's MPI_Alltoallw produced on host arrays
  (tests/golden/alltoallw_golden.json): a halo exchange (vector column face,
  contiguous row face, subarray ghost cells, nothing to self), a transpose
  (a different subarray per peer, received at odd byte displacements), unit
  widths 16, 4 and 1 in one pack launch, all-contiguous sides, every
  empty-segment position, IN_PLACE with a different derived type per peer.
  Each record is the whole receive allocation, prefilled with a
  position-dependent sentinel.
* Every refusal of mpigx_alltoallw, made by every rank in the same call: the
  error class, both allocations untouched, the next call still exact.
* On rank 0, after the collective cases: the segmented pack kernel alone
  (copy.hip segw_pack_kernel, through mpigx_pack_segments_w) against the numpy
  restatement of the type map at sizes taken from its launch geometry, 256
  threads per block and 4096 blocks dealt per launch, pack and unpack, with
  the unit width it chose for every segment.

n = 3 is in the default selection (one launch); n = 2 and 4, staging rounds
and the stream-ordered call are marked slow.  On the parent commit every one
fails: the mirror has no Alltoallw_."""
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
REFUSALS = ["null_sendcounts", "null_sdispls", "null_sendtypes", "null_recvcounts", "null_rdispls", "null_recvtypes",
            "negative_sendcount", "negative_recvcount", "unknown_type_in_an_empty_slot",
            "uncommitted_type_in_an_empty_slot", "freed_type_in_an_empty_slot", "unknown_sendtype", "null_recvbuf",
            "null_sendbuf", "null_comm", "refused_calls_wrote_nothing", "exact_after_refusals"]
GEOMETRY = [f"geometry_{g}_{d}" for g in ("unit_counts", "past_the_grid", "w16_beside_w1", "three_runs_straddle",
                                         "typed_base_lowers_w", "odd_pointer") for d in ("pack", "unpack")]


def run_worker(n, tmp_path, mode="full", **env):
    env = dict(ENV, DT_OUT=str(tmp_path / "aw"), ATW_MODE=mode, **env)
    rcs, outs = launch(os.path.join(ROOT, "tests", "spmd", "alltoallw_worker.py"), n, timeout=600, extra_env=env)
    recs = {}
    for r in range(n):
        p = tmp_path / f"aw.{r}"
        if p.exists():
            recs[r] = json.loads(p.read_text())
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}\n{recs.get(r, {}).get('failed')}"
                    for r, (rc, o) in enumerate(zip(rcs, outs)))
    assert all(rc == 0 for rc in rcs), msg
    print({r: recs[r].get("seconds") for r in sorted(recs)})  # seconds since each rank's start, per phase
    for r in range(n):
        assert recs[r]["device"] is True and recs[r]["failed"] is None
        for c in recs[r]["dev_checks"]:
            assert c["got"] == c["want"], (r, c["check"], c["got"], c["want"])
    return recs


def run_table(n, tmp_path):
    recs = run_worker(n, tmp_path)
    with open(os.path.join(ROOT, "tests", "golden", "alltoallw_golden.json")) as f:
        gold = json.load(f)["runs"][str(n)]
    for r in range(n):
        assert [c["check"] for c in recs[r]["dev_checks"]] == REFUSALS + (GEOMETRY if r == 0 else [])
        assert len(recs[r]["records"]) == len(gold[r])
        for got, want in zip(recs[r]["records"], gold[r]):
            assert got == want, (r, got["case"], got, want)


def test_alltoallw_device_matches_mpich_n3(tmp_path):
    """(~3 s) Alltoallw reproduces MPICH's records at n = 3, refuses what it must, and rank 0 checks the
    segmented pack kernel's geometry against the model (one launch)."""
    run_table(3, tmp_path)


@pytest.mark.slow
@pytest.mark.parametrize("n", [2, 4])
def test_alltoallw_device_matches_mpich(n, tmp_path):
    """(~6 s) The same at n = 2 and 4."""
    run_table(n, tmp_path)


@pytest.mark.slow
def test_alltoallw_crosses_staging_rounds(tmp_path):
    """(~3 s) A typed Alltoallw whose blocks are at least three rounds of a 4096-byte staging arena."""
    recs = run_worker(3, tmp_path, mode="rounds", MPIGX_STAGING_BYTES="4096")
    assert all([c["check"] for c in recs[r]["dev_checks"]] == ["rounds"] for r in range(3))


@pytest.mark.slow
def test_alltoallw_stream_ordered(tmp_path):
    """(~3 s) One stream-ordered call (set_blocking 0), checked after mpigx_comm_synchronize."""
    recs = run_worker(3, tmp_path, mode="stream")
    assert all([c["check"] for c in recs[r]["dev_checks"]] == ["stream_ordered"] for r in range(3))
