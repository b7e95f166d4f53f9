#!/usr/bin/env python3
"""Gatherv of matrix columns through a resized vector type against the same
packed bytes through a predefined type.

    python3 tools/gatherv_typed_bench.py <out_dir> <name> [--n 4] [--mib 64]

The launcher (this file, which never touches the GPU) starts n rank processes
of itself, all on one GPU.  The root gathers a row-major R x C float64 matrix
of `mib` MiB by columns: every rank sends its C/n columns as contiguous
column-major data, and the root receives
  (a) with recvtype = resized(vector(R, 1, C, DOUBLE), 0, 8), one instance per
      column, counts in columns — the typed path: one seg_pack_kernel launch
      unpacks the pooled temporary after the byte exchange;
  (b) with recvtype = DOUBLE into a contiguous buffer, counts in elements — the
      predefined path, the same bytes through the unchanged code.
Both in ONE process, alternating call by call: HIP events around each call on
the communicator's stream, warm-up and timed calls each, the max over ranks per
call, then median / min / max over the calls.  Writes
<out_dir>/<name>_gatherv_typed_n<n>_1gpu.json.
"""
import argparse
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    cols = [C // n] * n
    f8 = MPI.Datatype(np.float64)
    T = MPI.Types
    col = T.commit_(T.create_resized(T.create_vector(R, 1, C, f8), 0, 8))
    leaf = T.commit_(T.create_contiguous(R, f8))
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    send = torch.rand(cols[rank] * R, device=dev, generator=g, dtype=torch.float64)
    mat = torch.zeros(R * C, device=dev, dtype=torch.float64) if rank == 0 else None
    flat = torch.zeros(R * C, device=dev, dtype=torch.float64) if rank == 0 else None
    elems = [c * R for c in cols]

    def typed():
        MPI.Gatherv_(MPI.Buffer(send, cols[rank], leaf), MPI.Buffer(mat, C, col) if rank == 0 else None, cols, 0, comm)

    def plain():
        MPI.Gatherv_(send, flat, elems, 0, comm)

    for _ in range(args.warmup):
        typed()
        plain()
    torch.cuda.synchronize()
    ok = True
    if rank == 0:  # the typed result is the transpose of the predefined one
        ok = bool(torch.equal(mat.view(R, C), flat.view(C, R).t()))
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(args.iters)] for k in "ab"}
    dist.barrier()
    for i in range(args.iters):
        for k, f in (("a", typed), ("b", plain)):
            e0, e1 = ev[k][i]
            e0.record(stream)
            f()
            e1.record(stream)
    torch.cuda.synchronize()
    ms = torch.tensor([[x.elapsed_time(y) for x, y in ev[k]] for k in "ab"], dtype=torch.float64)
    dist.all_reduce(ms, op=dist.ReduceOp.MAX)  # per call, the slowest rank
    if rank == 0:
        def stats(v):
            v = sorted(v.tolist())
            return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}

        a, b = stats(ms[0]), stats(ms[1])
        print(json.dumps({"n": n, "gpus": 1, "ranks_share_one_gpu": True, "mib": args.mib, "R": R, "C": C,
                          "iters": args.iters, "warmup": args.warmup, "typed_equals_predefined_transposed": ok,
                          "gatherv_resized_vector_columns": a, "gatherv_predefined_same_bytes": b,
                          "typed_over_predefined_median": round(a["median_ms"] / b["median_ms"], 3),
                          "raw_ms": {"typed": [round(x, 4) for x in ms[0].tolist()],
                                     "predefined": [round(x, 4) for x in ms[1].tolist()]}}), flush=True)
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
               "--iters", str(args.iters), "--warmup", str(args.warmup)]
        log = open(os.path.join(outdir, f"gatherv_typed_n{n}_rank{r}.log"), "w")
        procs.append((subprocess.Popen(["timeout", "-k", "10", str(args.timeout), *cmd], env=env, cwd=ROOT, stdout=log,
                                       stderr=subprocess.STDOUT), log))
    rcs = []
    for p, log in procs:
        rcs.append(p.wait())
        log.close()
    if any(rcs):
        raise RuntimeError(f"ranks exited {rcs} (logs in {outdir})")
    for line in open(os.path.join(outdir, f"gatherv_typed_n{n}_rank0.log")):
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
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.rank_worker:
        return rank_main(args)
    os.makedirs(args.out_dir, exist_ok=True)
    res = launch(args.n, args, args.out_dir)
    with open(os.path.join(args.out_dir, f"{args.name}_gatherv_typed_n{args.n}_1gpu.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "raw_ms"}), flush=True)


if __name__ == "__main__":
    main()
