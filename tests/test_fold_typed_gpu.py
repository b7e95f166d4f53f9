"""The local fold through non-contiguous derived datatypes
(mpigx_reduce_local_multi / mpigx_reduce_local with a committed derived
handle; kernels.hpp fold_typed_kernel) against numpy: every input gathered
through the type map, folded in rank order by the oracle, scattered into a
copy of the output's initial image.  The whole allocation is compared, guard
bytes included: covered elements as the oracle's bits, every other byte
untouched."""
import ctypes
import os
import sys

import numpy as np
import pytest

from gen_inputs import make
from golden_io import same_bits
from oracle import mpich_model as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "spmd"))
import strided_cases as S  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
ERR_TYPE, ERR_OP, ERR_ARG = 3, 9, 12


def tmap(spec):
    """strided_cases.typemap plus ("struct", [(byte displacement, member)], extent)."""
    if isinstance(spec, np.dtype):
        return S.typemap(spec)
    if spec[0] == "struct":
        return np.concatenate([d + tmap(m)[0] for d, m in spec[1]]), 0, spec[2]
    if spec[0] == "resized":
        return tmap(spec[1])[0], spec[2], spec[3]
    return S.typemap(spec)


def build(L, spec, basic, commit=True):
    """The (committed) libmpigx handle of a spec over the predefined handle `basic`."""
    h = ctypes.c_int()
    ints = lambda xs: (ctypes.c_int * len(xs))(*xs)  # noqa: E731
    if isinstance(spec, np.dtype):
        return basic
    if spec[0] == "vector":
        rc = L.mpigx_type_vector(spec[1], spec[2], spec[3], build(L, spec[4], basic), ctypes.byref(h))
    elif spec[0] == "subarray":
        rc = L.mpigx_type_create_subarray(len(spec[1]), ints(spec[1]), ints(spec[2]), ints(spec[3]), 56,
                                          build(L, spec[4], basic), ctypes.byref(h))  # MPI_ORDER_C
    elif spec[0] == "resized":
        rc = L.mpigx_type_create_resized(build(L, spec[1], basic), spec[2], spec[3], ctypes.byref(h))
    else:
        mem = [build(L, m, basic) for _, m in spec[1]]
        s = ctypes.c_int()
        assert L.mpigx_type_create_struct(len(mem), ints([1] * len(mem)),
                                          (ctypes.c_longlong * len(mem))(*[d for d, _ in spec[1]]), ints(mem),
                                          ctypes.byref(s)) == 0
        rc = L.mpigx_type_create_resized(s.value, 0, spec[2], ctypes.byref(h))
    assert rc == 0
    if commit:
        assert L.mpigx_type_commit(ctypes.byref(h)) == 0
    return h.value


def case(dt, op, spec, counts, nins, off=0):
    return dict(dt=dt, op=op, spec=spec(np.dtype(M.DTYPES[dt][1])), counts=counts, nins=nins, off=off)


# T = kThreads * kFoldTypedU = 1024 units per block pass; the largest count of
# every case runs again with the grid capped to one block (the stride loop).
CASES = {
    # a column: element mode, one element per unit
    "column_i8": case("INT8_T", "BXOR", lambda o: ("vector", 7, 1, 3, o), (1, 147), (1, 2, 3)),
    # ... with the unit total at T - 1, T, T + 1 (one instance each)
    "column_T-1": case("FLOAT", "MAX", lambda o: ("vector", 1023, 1, 3, o), (1,), (2,)),
    "column_T": case("FLOAT", "MAX", lambda o: ("vector", 1024, 1, 3, o), (1,), (3,)),
    "column_T+1": case("FLOAT", "MAX", lambda o: ("vector", 1025, 1, 3, o), (1,), (2,)),
    # blocks of 32 B at 48 B: 16-B units on an aligned pointer (1030 at count 103), 4-B units 4 B off
    "blocks_16B": case("FLOAT", "SUM", lambda o: ("vector", 5, 8, 12, o), (1, 103), (2, 8)),
    "blocks_4B": case("FLOAT", "SUM", lambda o: ("vector", 5, 8, 12, o), (1, 103), (2, 16), off=4),
    # 3-D interior: 2 runs of 3 blocks of 8 B, 2-byte elements in 4-B units (packed pairs)
    "subarray_bf16": case("BFLOAT16", "SUM", lambda o: ("subarray", (4, 5, 8), (2, 3, 4), (1, 1, 2), o), (1, 44),
                          (3, 16)),
    # two vectors of different block lengths: prefix 0 / 48 / 128, searched
    "struct_i64": case("INT64_T", "MIN", lambda o: ("struct", [(0, ("vector", 3, 2, 4, o)),
                                                               (96, ("vector", 2, 5, 7, o))], 200), (1, 65), (2, 3)),
    # extent beyond the true extent, lb != 0, 16-byte elements 8 bytes off: moved in 8-byte pieces
    "resized_c128": case("C_DOUBLE_COMPLEX", "PROD", lambda o: ("resized", ("vector", 3, 1, 2, o), -16, 112), (1, 4),
                         (2, 3), off=8),
    # 70 runs (> kInlineRuns): the table is read from global memory
    "long_table": case("FLOAT", "MAX", lambda o: ("vector", 70, 1, 3, ("vector", 2, 1, 2, o)), (1, 9), (2,)),
    # row mode: 3 rows of 64 x 16 B + 4 elements at twice that stride
    "rows": case("FLOAT", "SUM", lambda o: ("vector", 3, 260, 520, o), (1, 5, 6), (1, 2, 8)),
}


@pytest.fixture(scope="module")
def L():
    import mpigx
    assert torch.cuda.is_available()
    return mpigx.lib()


def fold(L, ptrs, out, count, h, op, order):
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    return L.mpigx_reduce_local_multi(arr, len(ptrs), ctypes.c_void_p(out), count, h, M.OPS[op], order, None)


def refusals(L):
    f32, i32 = M.DTYPES["FLOAT"][0], M.DTYPES["INT32_T"][0]
    vec = ("vector", 3, 1, 2, np.dtype(np.float32))
    img = S.data(256, 5)
    bufs = [torch.from_numpy(img.copy()).cuda() for _ in range(4)]
    p = [b.data_ptr() for b in bufs]
    col = build(L, vec, f32)
    same = build(L, ("struct", [(0, np.dtype(np.float32)), (8, np.dtype(np.float32))], 16), f32)
    s = ctypes.c_int()  # ... and that struct over two predefined types
    assert L.mpigx_type_create_struct(2, (ctypes.c_int * 2)(1, 1), (ctypes.c_longlong * 2)(0, 8),
                                      (ctypes.c_int * 2)(f32, i32), ctypes.byref(s)) == 0
    assert L.mpigx_type_commit(ctypes.byref(s)) == 0
    assert fold(L, p[:2], p[3], 2, same, "SUM", 1) == 0  # one predefined type: accepted
    bufs[3].copy_(torch.from_numpy(img))
    assert fold(L, p[:3], p[3], 2, col, "SUM", 0) == ERR_ARG  # MPICH order over three typed leaves
    assert fold(L, p[:2], p[3], 2, s.value, "SUM", 1) == ERR_TYPE
    assert fold(L, p[:2], p[3], 2, col, "BAND", 1) == ERR_OP
    assert fold(L, p[:2], p[3], 2, build(L, vec, f32, commit=False), "SUM", 1) == ERR_TYPE
    assert L.mpigx_reduce_local(p[0], p[3], 2, s.value, M.OPS["SUM"]) == ERR_TYPE
    torch.cuda.synchronize()
    for b in bufs:
        assert np.array_equal(b.cpu().numpy(), img)


@pytest.mark.parametrize("name", list(CASES) + ["refusals"])
def test_fold_typed(L, name, monkeypatch):
    """(~0.5 s) Reduce_local through non-contiguous derived types, bit-exact against the
    oracle's rank-ordered fold over the numpy type map, gaps and guard bytes
    untouched; the refusals write nothing."""
    if name == "refusals":
        return refusals(L)
    c = CASES[name]
    dt, op, spec = c["dt"], c["op"], c["spec"]
    npdt, bf = np.dtype(M.DTYPES[dt][1]), dt == "BFLOAT16"
    h = build(L, spec, M.DTYPES[dt][0])
    cmax, nmax = max(c["counts"]), max(c["nins"])
    offs, _, ext = tmap(spec)
    base = GUARD + c["off"]
    nbytes = base + int(offs.max()) + 1 + (cmax - 1) * ext + GUARD
    addrs = lambda count: base + (np.arange(count)[:, None] * ext + offs[None, :]).reshape(-1)  # noqa: E731
    # inputs: valid elements everywhere the type reaches, a byte pattern elsewhere
    elems = make(dt, op, nmax, len(offs) * cmax // npdt.itemsize, 3, edge=True)
    imgs = [S.data(nbytes, k) for k in range(nmax)]
    for img, el in zip(imgs, elems):
        img[addrs(cmax)] = el.view(np.uint8)
    devs = [torch.from_numpy(img).cuda() for img in imgs]
    out0 = S.data(nbytes, 99)
    dout = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def check(start, parts, call, tag):
        """`call` on an output that starts as `start` leaves the fold of `parts` there and nothing else."""
        dout.copy_(torch.from_numpy(start))
        assert call(dout.data_ptr() + base) == 0, tag
        got, want = dout.cpu().numpy(), start.copy()
        want[a] = M.fold_linear([p[a].view(npdt) for p in parts], dt, op).view(np.uint8)
        assert same_bits(got[a].view(npdt), want[a].view(npdt), bf), tag
        got[a] = want[a]
        assert np.array_equal(got, want), tag  # gaps and guard bytes

    for count in c["counts"]:
        a = addrs(count)
        for nin in c["nins"]:
            ptrs = [d.data_ptr() + base for d in devs[:nin]]
            # LINEAR; at nin = 2 the MPICH order too (the same bits); the largest count on one block
            for order, cap in [(1, None)] + [(0, None)] * (nin == 2) + [(1, "1")] * (count == cmax):
                if cap:
                    monkeypatch.setenv("MPIGX_LOCAL_MAX_BLOCKS", cap)
                check(out0, imgs[:nin], lambda o: fold(L, ptrs, o, count, h, op, order), (name, count, nin, order, cap))
                monkeypatch.delenv("MPIGX_LOCAL_MAX_BLOCKS", raising=False)
        # MPI_Reduce_local itself: inout = op(inout, in), the inout typed and aliasing input 0
        check(imgs[0], imgs[:2], lambda o: L.mpigx_reduce_local(devs[1].data_ptr() + base, o, count, h, M.OPS[op]),
              (name, count, "reduce_local"))
