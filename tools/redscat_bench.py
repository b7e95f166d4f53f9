#!/usr/bin/env python3
"""Reduce_scatter_block against the Allreduce a caller had to use before it.

    python3 tools/redscat_bench.py <out_dir> <name> [--n 2,4,8] [--mib 256,16]

The launcher (this file, which never touches the GPU) starts n rank processes
of itself per rank count, all on one GPU with MPIGX_PEER_MEM=xdev (the
one-rank-per-GPU signalling).  Each rank times, for f32 SUM on a sendbuf of
`mib` MiB per rank, in ONE process and alternating call by call:
  (a) Reduce_scatter_block, zero-copy (the dedicated kernel);
  (b) Allreduce of the same sendbuf on the default path — what returns the
      same data without this call.
HIP events around each call on the communicator's stream, 3 warm-up and 20
timed calls each, the max over ranks per call, then median / min / max over
the calls, and one more call of (a) with the per-block phase stamps on.
Writes <out_dir>/<name>_redscat_n<n>_1gpu_xdev.json.

(a)'s read rate counts what a rank's kernel reads: (n-1)/n S from the peers'
buffers and S/n from its own.  With every rank on one GPU all of it is HBM
traffic of that GPU; over xGMI it is NOT measured here.
"""
import argparse
import ctypes
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
    res = []
    for mib in args.mib:
        count = (mib << 20) // 4 // n * n
        g = torch.Generator(device=dev).manual_seed(1000 + rank)
        send = torch.rand(count, device=dev, generator=g) * 2 - 1
        ar = torch.empty_like(send)
        rs = torch.empty(count // n, device=dev)
        # both sizes are at or above the default MPIGX_ZC_MIN (16 MiB): (a) runs its zero-copy kernel
        # and (b) the zero-copy two-shot the engine's tuner picks (its first calls time the variants)
        assert count * 4 >= MPI.get_knob(comm, "ZC_MIN") > 0
        for _ in range(args.warmup):
            MPI.Reduce_scatter_block_(send, rs, count // n, MPI.SUM, comm)
        for _ in range(args.warmup + 3):
            MPI.Allreduce_(send, ar, MPI.SUM, comm)
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(args.iters)] for k in "ab"}
        dist.barrier()
        for i in range(args.iters):
            a0, a1 = ev["a"][i]
            a0.record(stream)
            MPI.Reduce_scatter_block_(send, rs, count // n, MPI.SUM, comm)
            a1.record(stream)
            b0, b1 = ev["b"][i]
            b0.record(stream)
            MPI.Allreduce_(send, ar, MPI.SUM, comm)
            b1.record(stream)
        torch.cuda.synchronize()
        ms = torch.tensor([[x.elapsed_time(y) for x, y in ev[k]] for k in "ab"], dtype=torch.float64)
        dist.all_reduce(ms, op=dist.ReduceOp.MAX)  # per call, the slowest rank
        # one stamped call of (a)
        st = torch.zeros(1024 * 8, dtype=torch.int64, device=dev)
        MPI.lib().mpigx_comm_set_stamps(comm.val, ctypes.c_void_p(st.data_ptr()))
        MPI.Reduce_scatter_block_(send, rs, count // n, MPI.SUM, comm)
        torch.cuda.synchronize()
        MPI.lib().mpigx_comm_set_stamps(comm.val, None)
        t = st.view(1024, 8)[:, :6].cpu().numpy().astype(np.int64)
        t = t[t[:, 0] > 0]
        phases = {}
        if t.size:
            d = np.diff(t, axis=1) / 100.0
            phases = {"entry_barrier_us": round(float(np.median(d[:, 0])), 2), "fold_us": round(float(np.median(d[:, 1])), 2),
                      "fold_us_max": round(float(d[:, 1].max()), 2),
                      "exit_barrier_us": round(float(np.median(d[:, 4])), 2),
                      "span_us": round(float(t[:, 5].max() - t[:, 0].min()) / 100.0, 2), "blocks": int(t.shape[0])}
        allp = [None] * n
        dist.all_gather_object(allp, phases)
        if rank == 0:
            S = count * 4

            def stats(v):
                v = sorted(v.tolist())
                return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}

            a, b = stats(ms[0]), stats(ms[1])
            res.append({"mib": mib, "bytes_per_rank": S, "reduce_scatter_block_zc": a, "allreduce_default": b,
                        "speedup_median": round(b["median_ms"] / a["median_ms"], 3),
                        "a_read_GBps_per_rank_median": round(S / (a["median_ms"] / 1e3) / 1e9, 1),
                        "a_read_GBps_all_ranks_median": round(n * S / (a["median_ms"] / 1e3) / 1e9, 1),
                        "phases_us_per_rank": allp})
    if rank == 0:
        ranks_share, cap = MPI.device_share(comm)
        print(json.dumps({"n": n, "gpus": 1, "peer_mem": str(MPI.peer_memory(comm)), "dtype": "f32", "op": "SUM",
                          "iters": args.iters, "warmup": args.warmup, "grid_cap": cap, "ranks_per_device": ranks_share,
                          "read_rate_is": "HBM of the one GPU every rank shares; xGMI not measured",
                          "sizes": res}), flush=True)
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
                   MASTER_PORT=str(port), MPIGX_DEVICE="0", MPIGX_TIMEOUT_MS="20000", MPIGX_PEER_MEM="xdev")
        cmd = [sys.executable, os.path.abspath(__file__), "--rank-worker", "--mib", ",".join(map(str, args.mib)),
               "--iters", str(args.iters), "--warmup", str(args.warmup)]
        log = open(os.path.join(outdir, f"redscat_bench_n{n}_rank{r}.log"), "w")
        procs.append((subprocess.Popen(["timeout", "-k", "10", str(args.timeout), *cmd], env=env, cwd=ROOT, stdout=log,
                                       stderr=subprocess.STDOUT), log))
    rcs = []
    for p, log in procs:
        rcs.append(p.wait())
        log.close()
    if any(rcs):
        raise RuntimeError(f"ranks exited {rcs} (logs in {outdir})")
    for line in open(os.path.join(outdir, f"redscat_bench_n{n}_rank0.log")):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError(f"no result line (logs in {outdir})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?")
    ap.add_argument("name", nargs="?")
    ap.add_argument("--rank-worker", action="store_true")
    ap.add_argument("--n", default="2,4,8")
    ap.add_argument("--mib", default="256,16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    args.mib = [int(x) for x in args.mib.split(",")]
    if args.rank_worker:
        return rank_main(args)
    os.makedirs(args.out_dir, exist_ok=True)
    for n in (int(x) for x in args.n.split(",")):
        # a failed rank count ends the run: nothing more is started on the GPU
        res = launch(n, args, args.out_dir)
        path = os.path.join(args.out_dir, f"{args.name}_redscat_n{n}_1gpu_xdev.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        for s in res["sizes"]:
            print(f"n={n} {s['mib']} MiB: reduce_scatter_block {s['reduce_scatter_block_zc']}  allreduce "
                  f"{s['allreduce_default']}  x{s['speedup_median']}", flush=True)


if __name__ == "__main__":
    main()
