"""Reduce_scatter_block / Reduce_scatter without a GPU: the CPU restatement of
MPICH's fold order (tests/redscat_model.py) against the fixtures recorded from
MPICH 3.3.2 (tests/golden/redscat_golden*.npz), the fixtures' duty to
discriminate, and the argument checks that need no device."""
import ctypes
import os

import numpy as np
import pytest

import mpigx
import redscat_model as R
from mpigx import consts as C

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _nan_blind_equal(a, b):
    """Bitwise, except that any NaN matches any NaN (payload and sign of a
    generated NaN differ by ISA; tests/golden_io.py same_bits)."""
    if a.dtype.kind in "fc":
        fa, fb = a.view(a.real.dtype), b.view(b.real.dtype)
        na, nb = np.isnan(fa), np.isnan(fb)
        return a.shape == b.shape and np.array_equal(na, nb) and fa[~na].tobytes() == fb[~nb].tobytes()
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_covers_the_cases(golden):
    cases, arrays = golden
    assert sorted({c["n"] for c in cases}) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert sorted(arrays) == sorted(c["id"] for c in cases)
    for name, _ in R.GOLDEN_FILES:
        assert os.path.getsize(os.path.join(HERE, name)) < (1 << 20), name
    by_n = {n: [c for c in cases if c["n"] == n] for n in (1, 2, 3, 4, 5, 6, 7, 8)}
    for n, cs in by_n.items():
        assert {c["count"] for c in cs if not c["spans"]} == {1, 3, 1024}
        assert any(c["v"] and 0 in R.counts_of(c, n) for c in cs) or n == 1
        assert any(c["inplace"] and c["v"] for c in cs) and any(c["inplace"] and not c["v"] for c in cs)
        # the 512 KiB switch from both sides, per element size
        for dt, es in (("FLOAT", 4), ("UINT8_T", 1)):
            tot = sorted(c["count"] * n * es for c in cs if c["spans"] and c["dtype"] == dt)
            assert tot[0] < R.SWITCH <= tot[-1] and tot[-1] - tot[0] <= 2 * n * es
    n8 = sorted({c["count"] for c in by_n[8] if c["spans"] and c["dtype"] == "FLOAT"})
    n3 = sorted({c["count"] for c in by_n[3] if c["spans"] and c["dtype"] == "FLOAT"})
    assert n8 == [16383, 16384] and n3 == [43690, 43691]


def test_model_reproduces_every_fixture(golden):
    cases, arrays = golden
    bad = []
    for c in cases:
        n = c["n"]
        counts = R.counts_of(c, n)
        got = R.reduce_scatter(R.case_inputs(c), counts, c["dtype"], c["op"])
        want = R.split_outputs(c, arrays[c["id"]])
        for r in range(n):
            if not _nan_blind_equal(R.sample(got[r], c), want[r]):
                bad.append((c["id"], r))
    assert not bad, bad[:10]


def test_fixtures_discriminate(golden):
    """Every FLOAT SUM case at n >= 4: the rank-ordered left fold of the same
    inputs differs from MPICH's output somewhere.  Every MIN / MAX case on NaN
    or signed-zero inputs (n >= 2): the model with swapped operand roles does."""
    cases, arrays = golden
    nsum = nrole = 0
    for c in cases:
        n = c["n"]
        fsum = c["dtype"] == "FLOAT" and c["op"] == "SUM" and n >= 4
        roles = c["op"] in ("MIN", "MAX") and c["mode"] in (R.G_NAN, R.G_SZERO) and n >= 2
        if not (fsum or roles):
            continue
        counts = R.counts_of(c, n)
        ins = R.case_inputs(c)
        if fsum:
            other = R.reduce_scatter(ins, counts, c["dtype"], c["op"], order="linear")
            nsum += 1
        else:
            other = R.reduce_scatter(ins, counts, c["dtype"], c["op"], swap=True)
            nrole += 1
        want = R.split_outputs(c, arrays[c["id"]])
        assert any(not _nan_blind_equal(R.sample(other[r], c), want[r]) for r in range(n)), c["id"]
    assert nsum >= 4 * 8 and nrole >= 6 * 10


def _rs_objects():
    import glob
    return sorted(glob.glob(os.path.join(os.path.dirname(HERE), "..", "mpi.jl_amd", "build", "rs_*.o")))


@pytest.mark.skipif(not _rs_objects() or not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                    reason="kernel objects not built (run __graft_entry__.build())")
@pytest.mark.parametrize("obj", _rs_objects(), ids=[os.path.basename(o)[:-2] for o in _rs_objects()])
def test_rs_kernels_have_no_scratch(obj, tmp_path):
    """Every rs_kernel instantiation has a zero private segment, like its
    siblings (tests/test_kernel_resources_cpu.py): 5 shapes per schedule, 2
    schedules, per op."""
    from test_kernel_resources_cpu import _kernel_private_sizes
    sizes = {k: v for k, v in _kernel_private_sizes(obj, str(tmp_path)).items() if "9rs_kernel" in k}
    assert len(sizes) >= 20 and len(sizes) % 10 == 0, (obj, len(sizes))
    assert all(v == 0 for v in sizes.values()), {k: v for k, v in sizes.items() if v}


def test_null_comm_is_err_comm():
    L = mpigx.lib()
    assert L.mpigx_reduce_scatter_block(None, None, 1, C.MPI_FLOAT, C.MPI_SUM, None) == C.MPI_ERR_COMM
    cnt = (ctypes.c_int * 2)(1, 1)
    assert L.mpigx_reduce_scatter(None, None, cnt, C.MPI_FLOAT, C.MPI_SUM, None) == C.MPI_ERR_COMM


def test_counts_are_cints():
    """A count of 2^31 (or a total that reaches it) is Julia's InexactError
    before any call, in every form of the mirror."""
    from mpigx import api
    comm = api.Comm(None, 0, 2, None)
    buf = np.zeros(4, dtype=np.float32)
    with pytest.raises(api.InexactError):
        api.Reduce_scatter_block_(buf, buf, 1 << 31, mpigx.SUM, comm)
    with pytest.raises(api.InexactError):
        api.Reduce_scatter_block_(buf, 1 << 30, mpigx.SUM, comm)  # in place: 2 * 2^30 elements
    with pytest.raises(api.InexactError):
        api.Reduce_scatter_(buf, buf, [1 << 31, 0], mpigx.SUM, comm)
    with pytest.raises(api.InexactError):
        api.Reduce_scatter_(buf, [1 << 30, 1 << 30], mpigx.SUM, comm)
    for name in ("Reduce_scatter_block_", "Reduce_scatter_block", "Reduce_scatter_"):
        assert getattr(mpigx, name) is getattr(api, name)
