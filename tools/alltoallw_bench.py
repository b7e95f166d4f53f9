#!/usr/bin/env python3
"""Alltoallw against the typed Alltoallv it generalises, and the mixed-width
pack launch with and without its W = 1 neighbour.

    python3 tools/alltoallw_bench.py <out_dir> <name> [--n 4] [--mib 64]

The launcher (this file, which never touches the GPU) starts n rank processes
of itself, all on one GPU.

(1) Every rank holds a row-major R x C float64 matrix of `mib` MiB and sends
C/n of its columns to every peer, one resized(vector(R, 1, C, DOUBLE), 0, 8)
instance per column, received as contiguous columns:
  (a) `Alltoallw_` with that type in every slot, displacements in bytes: one
      segw_pack_kernel launch packs the pooled temporary before the exchange;
  (b) the existing typed `Alltoallv_` (seg_pack_kernel), the yardstick.
Both in ONE process, alternating call by call (--first w|v says which of the
pair goes first): HIP events around each call on
the communicator's stream, the max over ranks per call, then median / min /
max over the calls.

(2) On rank 0 alone, through mpigx_pack_segments_w: a W = 16 segment of
`mib` / 2 MiB packed alone, beside a W = 1 segment of 1 MiB in the same launch,
that W = 1 segment alone, and the W = 16 segment's layout at a typed address
that forces it down to W = 1 (what a launch-wide unit width would cost it).

Writes <out_dir>/<name>_alltoallw_n<n>_1gpu.json.
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def mixed_width(args, MPI, torch, dev):
    import numpy as np
    T = MPI.Types
    f8, u1 = MPI.Datatype(np.float64), MPI.Datatype(np.uint8)
    pairs = T.commit_(T.create_vector(2, 2, 4, f8))      # two 16-byte runs, extent 48: W = 16
    sparse = T.commit_(T.create_resized(u1, 0, 2))       # one byte out of two: W = 1
    big = (args.mib << 20) // 2 // 32                    # instances of `pairs`
    small = 1 << 20                                      # instances of `sparse`
    typed = torch.zeros(big * 48 + 2 * small + 64, device=dev, dtype=torch.uint8)
    packed = torch.zeros(big * 32 + small + 64, device=dev, dtype=torch.uint8)
    L = MPI.lib()
    LL = ctypes.c_longlong

    def launch(segs, base=0):
        k = len(segs)
        w = (ctypes.c_int * k)()
        a = ((ctypes.c_int * k)(*[s[0].val for s in segs]), (LL * k)(*[s[1] for s in segs]),
             (LL * k)(*[s[2] for s in segs]), (LL * k)(*[s[3] for s in segs]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for i in range(args.warmup + args.iters):
            e0.record()
            rc = L.mpigx_pack_segments_w(ctypes.c_void_p(typed.data_ptr() + base), k, *a,
                                         ctypes.c_void_p(packed.data_ptr()), 0, w, None)
            e1.record()
            assert rc == 0, rc
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(stats(ms), w=list(w))

    s16 = (pairs, big, 0, 0)
    s1 = (sparse, small, big * 48, big * 32)
    return {"w16_bytes": big * 32, "w1_bytes": small, "w16_alone": launch([s16]), "w16_beside_w1": launch([s16, s1]),
            "w1_alone": launch([s1]), "w16_layout_forced_to_w1": launch([s16], base=1)}


def rank_main(args):
    sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))
    import numpy as np
    import torch
    import torch.distributed as dist

    import mpigx as MPI

    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = MPI.Init()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    C = 4096
    R = (args.mib << 20) // 8 // C
    per = C // n
    f8 = MPI.Datatype(np.float64)
    T = MPI.Types
    col = T.commit_(T.create_resized(T.create_vector(R, 1, C, f8), 0, 8))
    leaf = T.commit_(T.create_contiguous(R, f8))
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    mat = torch.rand(R * C, device=dev, generator=g, dtype=torch.float64)
    out_w = torch.zeros(R * C, device=dev, dtype=torch.float64)
    out_v = torch.zeros(R * C, device=dev, dtype=torch.float64)
    counts = [per] * n

    def w():
        MPI.Alltoallw_(mat, counts, [q * per * 8 for q in range(n)], [col] * n,
                       out_w, counts, [p * per * R * 8 for p in range(n)], [leaf] * n, comm)

    def v():
        MPI.Alltoallv_(MPI.Buffer(mat, C, col), MPI.Buffer(out_v, C, leaf), counts, counts, comm)

    order = (("a", w), ("b", v)) if args.first == "w" else (("b", v), ("a", w))
    for _ in range(args.warmup):
        for _, f in order:
            f()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out_w, out_v)) and bool(torch.equal(
        out_w.view(n, per, R)[rank], mat.view(R, C)[:, rank * per:(rank + 1) * per].t()))
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(args.iters)] for k in "ab"}
    dist.barrier()
    for i in range(args.iters):
        for k, f in order:
            e0, e1 = ev[k][i]
            e0.record(stream)
            f()
            e1.record(stream)
    torch.cuda.synchronize()
    ms = torch.tensor([[x.elapsed_time(y) for x, y in ev[k]] for k in "ab"], dtype=torch.float64)
    dist.all_reduce(ms, op=dist.ReduceOp.MAX)  # per call, the slowest rank
    oks = torch.tensor([int(ok)])
    dist.all_reduce(oks, op=dist.ReduceOp.MIN)
    dist.barrier()
    if rank == 0:
        a, b = stats(ms[0]), stats(ms[1])
        mixed = mixed_width(args, MPI, torch, dev)
        print(json.dumps({"n": n, "gpus": 1, "ranks_share_one_gpu": True, "mib_per_rank": args.mib, "R": R, "C": C,
                          "iters": args.iters, "warmup": args.warmup, "first_of_each_pair": args.first,
                          "alltoallw_equals_alltoallv": bool(oks.item()),
                          "alltoallw_resized_vector_columns": a, "alltoallv_typed_same_bytes": b,
                          "alltoallw_over_alltoallv_median": round(a["median_ms"] / b["median_ms"], 3),
                          "mixed_width_pack": mixed,
                          "raw_ms": {"alltoallw": [round(x, 4) for x in ms[0].tolist()],
                                     "alltoallv": [round(x, 4) for x in ms[1].tolist()]}}), flush=True)
    dist.barrier()
    MPI.Finalize()
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(n, args, outdir):
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), MPIGX_DEVICE="0", MPIGX_TIMEOUT_MS="20000")
        cmd = [sys.executable, os.path.abspath(__file__), "--rank-worker", "--mib", str(args.mib),
               "--iters", str(args.iters), "--warmup", str(args.warmup), "--first", args.first]
        log = open(os.path.join(outdir, f"alltoallw_n{n}_rank{r}.log"), "w")
        procs.append((subprocess.Popen(["timeout", "-k", "10", str(args.timeout), *cmd], env=env, cwd=ROOT, stdout=log,
                                       stderr=subprocess.STDOUT), log))
    rcs = []
    for p, log in procs:
        rcs.append(p.wait())
        log.close()
    if any(rcs):
        raise RuntimeError(f"ranks exited {rcs} (logs in {outdir})")
    for line in open(os.path.join(outdir, f"alltoallw_n{n}_rank0.log")):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError(f"no result line (logs in {outdir})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?")
    ap.add_argument("name", nargs="?")
    ap.add_argument("--rank-worker", action="store_true")
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--first", choices=("w", "v"), default="w", help="which call goes first in each timed pair")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.rank_worker:
        return rank_main(args)
    os.makedirs(args.out_dir, exist_ok=True)
    res = launch(args.n, args, args.out_dir)
    with open(os.path.join(args.out_dir, f"{args.name}_alltoallw_n{args.n}_1gpu.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "raw_ms"}), flush=True)


if __name__ == "__main__":
    main()
