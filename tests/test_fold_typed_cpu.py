"""mpigx_reduce_local / mpigx_reduce_local_multi with a derived datatype: the
argument refusals that return before any device call (no GPU needed)."""
import ctypes

import pytest

import mpigx
from mpigx import consts as C


@pytest.fixture(scope="module")
def L():
    return mpigx.lib()


def column(L, commit=True):
    h = ctypes.c_int()
    assert L.mpigx_type_vector(3, 1, 2, C.MPI_FLOAT, ctypes.byref(h)) == 0
    if commit:
        assert L.mpigx_type_commit(ctypes.byref(h)) == 0
    return h


def multi(L, nin, count, h, op=C.MPI_SUM, order=C.MPIGX_ORDER_LINEAR):
    ptrs = (ctypes.c_void_p * 17)(*[0x1000] * 17)  # never dereferenced
    return L.mpigx_reduce_local_multi(ptrs, nin, ctypes.c_void_p(0x1000), count, h, op, order, None)


def test_derived_type_refusals(L):
    col = column(L)
    assert multi(L, 2, 0, col.value) == 0  # nothing to do
    assert multi(L, 2, -1, col.value) == C.MPI_ERR_COUNT
    assert L.mpigx_reduce_local(None, None, -1, col.value, C.MPI_SUM) == C.MPI_ERR_COUNT
    assert multi(L, 2, (1 << 31) // 3 + 1, col.value) == C.MPI_ERR_COUNT  # 3 elements per instance
    for nin in (0, 17):
        assert multi(L, nin, 1, col.value) == C.MPI_ERR_ARG
    assert multi(L, 3, 1, col.value, order=C.MPIGX_ORDER_MPICH) == C.MPI_ERR_ARG
    assert multi(L, 2, 1, col.value, order=7) == C.MPI_ERR_ARG
    assert multi(L, 2, 1, col.value, op=C.MPI_BAND) == C.MPI_ERR_OP
    assert multi(L, 2, 1, column(L, commit=False).value) == C.MPI_ERR_TYPE
    foreign = ctypes.c_int((0x8C000000 | 3) - (1 << 32)).value  # a derived handle of MPICH's
    assert multi(L, 2, 1, foreign) == C.MPI_ERR_TYPE
    assert L.mpigx_reduce_local(None, None, 1, foreign, C.MPI_SUM) == C.MPI_ERR_TYPE
    freed = col.value
    assert L.mpigx_type_free(ctypes.byref(col)) == 0
    assert multi(L, 2, 1, freed) == C.MPI_ERR_TYPE
    assert L.mpigx_reduce_local(None, None, 1, freed, C.MPI_SUM) == C.MPI_ERR_TYPE
