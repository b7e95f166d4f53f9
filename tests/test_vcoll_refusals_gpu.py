"""What Gather, Gatherv, Scatter, Scatterv, Allgatherv and Alltoallv refuse on
device buffers, and with which error class (tests/spmd/vcoll_refusals_worker.py,
one three-rank launch, raw C ABI): null communicator, root out of range,
IN_PLACE at a non-root, null count / displacement arrays, negative counts,
unknown / uncommitted / freed type handles, null buffers.  Every row is made
with int32 on both sides and with a non-contiguous vector on one side, so the
in-place and the packed side give the same answer; every rank makes the same
refused call.  Afterwards the guard-padded allocations the calls pointed into
are unchanged and a valid Alltoallv is exact.

The expected classes are literal in the worker's table.  The rows of TIGHTENED
are the ones the v-collectives did not always refuse: with predefined types a
null buffer went to vx_kernel unless the rank's own block was non-empty
(Allgatherv) or unconditionally (Alltoallv).  Now a null buffer of a side with
any non-empty block is MPI_ERR_BUFFER on every route ("Refusals of
the v-collectives")."""
import json
import os

import pytest

from spmd_launch import ROOT, launch

pytestmark = pytest.mark.gpu

ENV = {"MPIGX_DEVICE": "0", "MPIGX_INIT_TIMEOUT_MS": "60000", "MPIGX_MAX_BLOCKS": "16", "MPIGX_TIMEOUT_MS": "30000",
       "MPIGX_STAGING_BYTES": str(32 << 20)}
TIGHTENED = ["allgatherv_null_recvbuf_peers_only_i4", "alltoallv_null_recvbuf_i4", "alltoallv_null_sendbuf_i4"]
# Gather / Scatter 17 rows each (their null-buffer row is int32 only), Gatherv / Scatterv 18, Allgatherv 28,
# Alltoallv 30
ROWS = 2 * 17 + 2 * 18 + 28 + 30


def test_vcollectives_refuse_alike_on_both_routes_n3(tmp_path):
    """(~4 s) Every refusal of the six calls at n = 3, int32 and vector variant; nothing written; the next call
    exact (one launch)."""
    n = 3
    env = dict(ENV, DT_OUT=str(tmp_path / "vr"))
    rcs, outs = launch(os.path.join(ROOT, "tests", "spmd", "vcoll_refusals_worker.py"), n, timeout=120, extra_env=env)
    recs = {r: json.loads((tmp_path / f"vr.{r}").read_text()) for r in range(n) if (tmp_path / f"vr.{r}").exists()}
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}\n{recs.get(r, {}).get('failed')}"
                    for r, (rc, o) in enumerate(zip(rcs, outs)))
    assert all(rc == 0 for rc in rcs), msg
    print({r: recs[r]["seconds"] for r in sorted(recs)})  # seconds since each rank's start, per phase
    for r in range(n):
        assert recs[r]["failed"] is None
        names = [c["check"] for c in recs[r]["checks"]]
        assert len(names) == len(set(names)) == ROWS + 2, (r, len(names))
        assert names[-2:] == ["refused_calls_wrote_nothing", "exact_after_refusals"]
        assert set(TIGHTENED) <= set(names)
        wrong = [(c["check"], c["got"], c["want"]) for c in recs[r]["checks"] if c["got"] != c["want"]]
        assert not wrong, (r, wrong)
