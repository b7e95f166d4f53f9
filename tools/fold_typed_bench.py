#!/usr/bin/env python3
"""Reduce_local through a non-contiguous derived type in one pass
(fold_typed_kernel) against what a caller could do before it: pack both
operands, fold the packed streams, unpack the result.

    python3 tools/fold_typed_bench.py <out_dir> <name> [--mib 64]

Two layouts of float32, `mib` MiB of packed data per operand:
  column: vector(n, 1, 8) — one element out of eight, element mode;
  rows:   vector(n, 1024, 2048) — rows of 4 KiB at a stride of 8 KiB, row mode.
Per layout, in ONE process and alternating call by call:
  (a) mpigx_reduce_local_multi([inout, in] -> inout) with the derived type;
  (b) mpigx_pack of inout and of in, the contiguous mpigx_reduce_local_multi
      on the packed streams, mpigx_unpack into inout.
HIP events around each on the null stream after warm-up; median / min / max
over the calls.  From traffic alone (a) moves 3 streams of packed size and
(b) 3 + 2 * 3.  Both results are compared bit for bit before timing.

Writes <out_dir>/<name>_fold_typed_1gpu.json.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def layout(args, MPI, torch, dev, blocklen, stride):
    import numpy as np
    L, T = MPI.lib(), MPI.Types
    f4 = MPI.Datatype(np.float32)
    elems = (args.mib << 20) // 4
    nblk = elems // blocklen
    dt = T.commit_(T.create_vector(nblk, blocklen, stride, f4))
    g = torch.Generator(device=dev).manual_seed(7)
    a0 = torch.rand(nblk * stride, device=dev, generator=g, dtype=torch.float32)
    b = torch.rand(nblk * stride, device=dev, generator=g, dtype=torch.float32)
    a, a2 = a0.clone(), a0.clone()
    pa, pb = torch.empty(elems, device=dev, dtype=torch.float32), torch.empty(elems, device=dev, dtype=torch.float32)
    vp = ctypes.c_void_p
    from mpigx import consts
    SUM, LINEAR = consts.MPI_SUM, consts.MPIGX_ORDER_LINEAR

    def multi(x, y, count, h):
        ptrs = (vp * 2)(x.data_ptr(), y.data_ptr())
        assert L.mpigx_reduce_local_multi(ptrs, 2, vp(x.data_ptr()), count, h, SUM, LINEAR, None) == 0

    def fused(x=a):
        multi(x, b, 1, dt.val)

    def three_step(x=a2):
        for t, p in ((x, pa), (b, pb)):
            pos = ctypes.c_longlong(0)
            assert L.mpigx_pack(vp(t.data_ptr()), 1, dt.val, vp(p.data_ptr()), elems * 4, ctypes.byref(pos), None) == 0
        multi(pa, pb, elems, f4.val)
        pos = ctypes.c_longlong(0)
        assert L.mpigx_unpack(vp(pa.data_ptr()), elems * 4, ctypes.byref(pos), vp(x.data_ptr()), 1, dt.val, None) == 0

    fused()
    three_step()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.view(torch.int32), a2.view(torch.int32))) and not bool(torch.equal(a, a0))
    ms = {"fused": [], "three_step": []}
    order = (("fused", fused), ("three_step", three_step))
    for i in range(args.warmup + args.iters):
        for k, f in (order if i % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    fu, th = stats(ms["fused"]), stats(ms["three_step"])
    gb = 3 * elems * 4 / 1e9
    return {"blocklen": blocklen, "stride": stride, "blocks": nblk, "packed_mib": args.mib, "same_bits": same,
            "fused": fu, "three_step": th, "fused_packed_GBps": round(gb / (fu["median_ms"] / 1e3), 1),
            "three_step_over_fused_median": round(th["median_ms"] / fu["median_ms"], 3),
            "raw_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("name")
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))
    import torch

    import mpigx as MPI
    if not torch.cuda.is_available():
        raise SystemExit("fold_typed_bench needs a GPU")
    dev = torch.device("cuda:0")
    res = {"mib": args.mib, "iters": args.iters, "warmup": args.warmup, "dtype": "float32", "op": "SUM",
           "column": layout(args, MPI, torch, dev, 1, 8), "rows": layout(args, MPI, torch, dev, 1024, 2048)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, f"{args.name}_fold_typed_1gpu.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: ({x: y for x, y in v.items() if x != "raw_ms"} if isinstance(v, dict) else v)
                      for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
