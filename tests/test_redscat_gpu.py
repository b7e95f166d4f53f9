"""Reduce_scatter_block / Reduce_scatter on device buffers, bit for bit
(tests/spmd/redscat_worker.py): the fixtures recorded from MPICH 3.3.2 on the
staged and the zero-copy path, large blocks against the model, LINEAR order,
bf16, derived types, user ops, error classes, cross-device signalling and
stream-ordered mode.

All ranks share cuda:0 on the 1-GPU test box; MPIGX_MAX_BLOCKS=16 keeps every
rank's grid co-resident (see test_collectives_gpu.py).  Process start
dominates every case here, so each test is one worker launch that runs both
paths: the zero-copy kernel is forced with the ZC_MIN=1 / ZC_REQUIRE=1 knobs
(the MPIGX_ZC_MIN / MPIGX_ZC_REQUIRE settings) inside the worker.
"""
import json
import os

import pytest

from spmd_launch import ROOT, launch
from test_collectives_gpu import ENV

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "spmd", "redscat_worker.py")


def _run(n, phase, min_checks, **extra):
    env = dict(ENV, RS_PHASE=phase, **extra)
    rcs, outs = launch(WORKER, n, timeout=300, extra_env=env)
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}" for r, (rc, o) in enumerate(zip(rcs, outs)))
    assert all(rc == 0 for rc in rcs), msg
    summ = [json.loads(l) for o in outs for l in o.splitlines() if l.startswith("{") and '"checks"' in l]
    assert len(summ) == n and all(x["nfail"] == 0 and x["checks"] >= min_checks for x in summ), summ
    return summ


@pytest.mark.parametrize("n", [2, 3, 5, 6, 7, 8])
def test_fixtures_staged_and_zero_copy(n):
    """(~25 s) Every MPICH fixture case at this n on the default (staged) path, then again through
    the dedicated zero-copy kernel: NMAX 2 / 4 / 8, full and pre-step shapes (rem 1 at n = 3 and 5,
    rem 2 at n = 6, rem 3 at n = 7), odd counts (misaligned blocks), a zero-count rank, both schedules across the
    512 KiB switch, and the in-place barrier rule."""
    summ = _run(n, "golden", 200, RS_ZC="1")
    assert all(x["zc_exchanges"] > 0 for x in summ), summ


@pytest.mark.parametrize("n", [4, 5])
def test_large_blocks_against_the_model(n):
    """(~13 s) 1 Mi + 3 elements per block (many blocks, a ragged last slice, no vector multiple),
    FLOAT SUM and INT64_T BAND, block and v forms, in place and out of place: staged in at least two
    rounds (a 16 MiB arena for 8 MiB blocks of INT64), then zero-copy.  In place also with strongly
    unequal counts ([1, M, M + 1, ...] and its mirror), where the stored region is input that other
    blocks still read and only the whole-launch barrier orders the two."""
    _run(n, "big", 28, MPIGX_STAGING_BYTES=str(16 << 20))


def test_orders_types_user_ops_and_errors():
    """(~4 s) n = 3: MPIGX_ORDER_LINEAR equals the sliced LINEAR fold; bf16 SUM / MAX equal the model;
    a contiguous derived type of 4 FLOATs; a non-commutative user op (affine maps on wrapping INT64
    pairs) through mpigx_op_create and mpigx_op_create_device against numpy in rank order; the error
    classes come back on every rank without hanging a peer."""
    _run(3, "misc", 29)


@pytest.mark.parametrize("n", [2, 4])
def test_cross_device_signalling(n):
    """(~7 s) MPIGX_PEER_MEM=xdev (the production one-rank-per-GPU signalling): 3 and 16384 per block
    FLOAT SUM on both paths."""
    _run(n, "xdev", 4, MPIGX_PEER_MEM="xdev")


def test_stream_ordered():
    """(~4 s) n = 2, set_blocking(0): two back-to-back calls on a side stream behind a producer
    kernel, then mpigx_comm_synchronize; exact results on both paths."""
    _run(2, "stream", 4)
