"""Index arithmetic of the derived-datatype kernels of the v-collectives and
of Get / Put (copy.hip seg_pack_kernel, typed_xfer_kernel) against the numpy
restatement of the type map (strided_cases.py), in one process on one GPU.
Sizes come from the kernels' launch geometry: 256 threads per block, 4096
blocks dealt per launch, unit widths W = 1, 2, 4, 8, 16.  The segmented kernel
is driven through mpigx_pack_segments (include/mpigx_diag.h), the transfer
kernel through Get and Put on this rank's own window."""
import ctypes
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpigx as MPI  # noqa: E402
import strided_cases as SC  # noqa: E402

comm = MPI.Init()
dev = torch.device(f"cuda:{comm.device}")
L = MPI.lib()
CASES = 0


def _ll(xs):
    return (ctypes.c_longlong * len(xs))(*[int(x) for x in xs])


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def main():
    global CASES
    # ---- segmented pack / unpack -------------------------------------------------
    # one unit per instance (an element every other slot), so a segment's unit
    # count is its instance count: empty, one unit, and one short of / exactly /
    # one past one, two and four 256-thread blocks; the packed boundaries of
    # the segments (prefix sums of these) all fall inside a block
    counts = [0, 1, 255, 256, 257, 511, 513, 1023, 1025]
    for W, el in ((1, "u1"), (2, "i2"), (4, "i4"), (8, "i8"), (16, "c16")):
        el = np.dtype(el)
        holes = ("resized", el, 0, 2 * W)
        # 6 runs of 2 blocks of 2 elements: the run search takes every branch
        runs6 = ("subarray", (6, 3, 4), (6, 2, 2), (0, 1, 1), el)
        cases = [(holes, counts)]
        cases.append((runs6, [0, 1, 2, 11, 0, 7]))
        if W == 1:  # past the 4096-block deal: every block loops over its share
            cases.append((holes, [3, 4096 * 256 + 300, 0, 513]))
        for spec, cnt in cases:
            ext, size = SC.typemap(spec)[2], SC.size_of(spec)
            dsp, offs, d, o = [], [], 1, 0
            for c in cnt:  # typed blocks one instance apart, packed blocks W bytes apart
                dsp.append(d)
                offs.append(o)
                d += c + 1
                o += c * size + W
            typed = SC.data(d * ext + 64, W)
            t_typed, t_pack = up(typed), up(SC.blank(o + 64))
            dt = SC.build(MPI, spec)
            args = (dt.val, len(cnt), _ll(cnt), _ll(dsp), _ll(offs))
            assert L.mpigx_pack_segments(ctypes.c_void_p(t_typed.data_ptr()), *args,
                                         ctypes.c_void_p(t_pack.data_ptr()), 0, None) == 0
            want = SC.blank(o + 64)
            for c, dd, oo in zip(cnt, dsp, offs):
                want[oo:oo + c * size] = SC.pack(typed, spec, c, dd)
            got = down(t_pack)
            CASES += 1
            assert np.array_equal(got, want), (W, spec[0], "pack", int(np.argmax(got != want)))
            t_back = up(SC.blank(len(typed)))
            assert L.mpigx_pack_segments(ctypes.c_void_p(t_back.data_ptr()), *args,
                                         ctypes.c_void_p(t_pack.data_ptr()), 1, None) == 0
            wantb = SC.blank(len(typed))
            for c, dd in zip(cnt, dsp):
                SC.unpack(wantb, SC.pack(typed, spec, c, dd), spec, c, dd)
            got = down(t_back)
            CASES += 1
            assert np.array_equal(got, wantb), (W, spec[0], "unpack", int(np.argmax(got != wantb)))

    # ---- typed transfer: Get and Put on this rank's own window -------------------
    for W, el in ((1, "u1"), (2, "i2"), (4, "i4"), (8, "i8"), (16, "c16")):
        el = np.dtype(el)
        runs6 = ("subarray", (6, 3, 4), (6, 2, 2), (0, 1, 1), el)   # 24 elements per instance
        holes = ("resized", ("vector", 3, 1, 2, el), 0, 6 * W)       # 3 elements per instance
        # (target instances, origin instances): one unit short of / exactly / past a block, several blocks
        shapes = [(1, 8), (32, 256), (33, 264)]
        if W == 1:
            shapes.append((43700, 349600))  # 1 048 800 units: past the 4096-block grid
        for tc, oc in shapes:
            nb = tc * SC.size_of(runs6)
            assert nb == oc * SC.size_of(holes)
            wbytes = SC.span(runs6, tc)[1] + 64
            obytes = SC.span(holes, oc)[1] + 64
            disp = 16
            win_np = SC.data(wbytes + disp, W + 1)
            win_t = up(win_np)
            win = MPI.Win_create(win_t, comm)
            MPI.Win_fence(0, win)
            o_t = up(SC.blank(obytes))
            MPI.Get(MPI.Buffer(o_t, oc, SC.build(MPI, holes)), oc, 0, disp, win, target=(tc, SC.build(MPI, runs6)))
            MPI.Win_fence(0, win)
            want = SC.blank(obytes)
            SC.unpack(want, SC.pack(win_np[disp:], runs6, tc), holes, oc)
            got = down(o_t)
            CASES += 1
            assert np.array_equal(got, want), (W, tc, "get", int(np.argmax(got != want)))
            src_np = SC.data(obytes, W + 2)
            src_t = up(src_np)
            MPI.Put(MPI.Buffer(src_t, oc, SC.build(MPI, holes)), oc, 0, disp, win,
                    target=(tc, SC.build(MPI, runs6)))
            MPI.Win_fence(0, win)
            wantw = win_np.copy()
            SC.unpack(wantw[disp:], SC.pack(src_np, holes, oc), runs6, tc)
            got = down(win_t)
            CASES += 1
            assert np.array_equal(got, wantw), (W, tc, "put", int(np.argmax(got != wantw)))
            MPI.free(win)


failed = None
try:
    main()
except Exception:  # noqa: BLE001
    failed = traceback.format_exc()
with open(f"{os.environ['DT_OUT']}.0", "w") as f:
    f.write(json.dumps({"failed": failed, "cases": CASES}) + "\n")
MPI.Finalize()
sys.exit(1 if failed else 0)
